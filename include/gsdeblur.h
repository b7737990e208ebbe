/* gsdeblur.h — C ABI of libgsdeblur_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the ONE hot path of SpectacularAI/3dgs-deblur:
 * differentiable 3DGS rasterization with motion-blur / rolling-shutter sub-frame
 * averaging.  In the reference the device side of this path is the torch C++/CUDA
 * extension `gsplat.cuda._C` of the SpectacularAI gsplat fork, called from the
 * Python autograd.Functions project_gaussians / rasterize_gaussians /
 * spherical_harmonics, which the nerfstudio fork's SplatfactoModel.get_outputs calls
 * once per training step.  Neither fork is vendored in the reference tree:
 *   /root/reference/.gitmodules:1-6          (declares the two submodules; dirs are empty)
 *   /root/reference/scripts/install.sh:10-22 (editable installs of both forks)
 *   /root/reference/README.md:199            (pin: nerfstudio 1.1.0, gsplat 409bcd3c ~ 0.1.11)
 *   /root/reference/train.py:115-122         (`ns-train splatfacto ... rasterize-mode antialiased`)
 *   /root/reference/render_model.py:11-15,217 (SplatfactoModel.get_outputs_for_camera)
 * so each entry point below cites the upstream-gsplat-0.1.11 interface it replaces
 * (recollected) plus the in-tree line that proves the path needs it.
 *
 * Conventions: every pointer is a DEVICE pointer unless marked "host"; all arrays are
 * contiguous; fp32/int32 unless noted; `stream` is a hipStream_t (NULL = default stream).
 * The library allocates nothing: outputs and workspaces are caller-owned.  No global state;
 * safe to call concurrently on different streams.  Return value: 0 = ok, 1 = invalid
 * argument, 3 = workspace too small, 1000+e = hipError_t e from the launch.
 *
 * Rasterizer record ("records"): 16 floats (64 bytes) per (sub-pose p, Gaussian g), index p*N+g:
 *   [0]x [1]y [2]conic.x [3]conic.y [4]conic.z [5]opacity [6]r [7]g [8]b [9]depth
 *   [10] int bits: tile_min.x | tile_min.y<<16   [11] int bits: tile_max.x | tile_max.y<<16
 *   [12] nmid = log2(255 * opacity) / 2   [13] kmul = opacity * 2^-nmid
 *   [14] qx = -log2(e)/2 * conic.x        [15] qz = -log2(e)/2 * conic.z
 *   ([12..15]: per-entry constants of the compositors' validity test |u| <= nmid and of alpha = kmul * 2^u,
 *    u = the exponent of alpha shifted by nmid; written by the projection / gs_pack_records; opacity < 1/255: nmid = -1)
 * Gradient records / tuples: 12 floats, slots 0..8 of the same layout; 11: d loss / d depth when a depth gradient is
 * present (gs_frame_backward_depth).  Slots 9 and 10 depend on the compositor that wrote them:
 *   exact rolling shutter / shared list (gs_rasterize_bwd_rs_slice): d loss / d pixel velocity (x, y), read by
 *     gs_project_pixvel_bwd with grad flag 16;
 *   SE(3) compositors with bwd_variant bit GS_BWD_ABSGRAD: "absgrad", the sums over the pixels of |d loss / d x| and
 *     |d loss / d y| of each (pixel, Gaussian) pair — the absolute value taken per pair and per component BEFORE any
 *     sum — read by gs_xy_absgrad_sum alone (the projection backwards ignore them);
 *   SE(3) compositors without that bit: unwritten, and nobody reads their sums.
 */
#ifndef GSDEBLUR_H
#define GSDEBLUR_H

#ifdef __cplusplus
extern "C" {
#endif

/* bwd_variant bit of gs_rasterize_bwd_slice / gs_frame_backward / gs_frame_backward_depth: run the absgrad
 * specialisations of the backward compositor (tuple form, otherwise-default variant: + 256 is allowed, the round-1 and
 * splat-parallel forms are refused; SE(3) frames only — the one rule that decides what runs and what is refused is the
 * dispatch block of gs_rasterize_bwd_slice_depth, csrc/raster_bwd.hip).  A variant bit and not a sibling entry point: the request changes
 * which compositor instantiation runs and nothing else — no new argument travels with it — which is what the variant
 * word already selects, so every existing prototype stays as it is. */
#define GS_BWD_ABSGRAD 2048

const char* gs_version(void);

/* ---- sub-pose schedule: SE(3) screw interpolation (north_star) --------------
 * viewmat(t_p) = Exp(-t_p * [lin_vel; ang_vel]) * viewmat, body twist in the OpenCV camera frame.
 * Velocity convention: /root/reference/process_synthetic_inputs.py:157-165,
 * /root/reference/render_video.py:100-115.  Config knobs: train.py:22,46,51,56. */
int gs_subpose_viewmats_fwd(int P, const float* viewmat /*16*/, const float* lin_vel /*3*/,
                            const float* ang_vel /*3*/, const float* times /*P*/,
                            float* out_viewmats /*P*16*/, void* stream);
/* v_viewmat[16], v_lin[3], v_ang[3] are accumulated into (caller zeroes them). */
int gs_subpose_viewmats_bwd(int P, const float* viewmat, const float* lin_vel, const float* ang_vel,
                            const float* times, const float* v_out /*P*16*/, float* v_viewmat,
                            float* v_lin, float* v_ang, void* stream);
/* the same sums STORED: v_viewmat[16] (row 3 = 0), v_lin[3], v_ang[3] may be uninitialised; every float is written, with
 * the bits gs_subpose_viewmats_bwd leaves in zeroed buffers (no fill launch in front of a one-block kernel) */
int gs_subpose_viewmats_bwd_store(int P, const float* viewmat, const float* lin_vel, const float* ang_vel,
                                  const float* times, const float* v_out /*P*16*/, float* v_viewmat,
                                  float* v_lin, float* v_ang, void* stream);
/* gs_subpose_viewmats_bwd_store plus the gradient of the sub-pose TIMES: v_times[p] = sum over the 12 entries of rows
 * 0..2 of v_out[p][j] * dV_p[j]/dt_p (dV_p/dt_p = -xi^ V_p, xi^ = [[ang]x lin; 0 0]).  All 22 + P floats are stored
 * (nothing to zero); v_viewmat, v_lin, v_ang hold exactly the bits gs_subpose_viewmats_bwd_store writes; v_times has one
 * writer per element and no reduction over p.  P <= 0 or a null output: GS_ERR_INVALID.  What learnable exposure and
 * readout times are trained through (SplatfactoDeblurConfig.camera_shutter_optimizer). */
int gs_subpose_viewmats_bwd_times(int P, const float* viewmat, const float* lin_vel, const float* ang_vel,
                                  const float* times, const float* v_out /*P*16*/, float* v_viewmat /*16*/,
                                  float* v_lin /*3*/, float* v_ang /*3*/, float* v_times /*P*/, void* stream);

/* ---- gsplat.project_gaussians (upstream _C.project_gaussians_forward/backward; SURVEY §8 a1,a3)
 * needed by: train.py:40 (camera-optimizer => viewmat grads), train.py:119 (antialiased => comp). */
int gs_project_fwd(int N, const float* means3d /*N*3*/, const float* scales /*N*3*/, float glob_scale,
                   const float* quats /*N*4 wxyz*/, const float* viewmat /*16*/, float fx, float fy,
                   float cx, float cy, int img_height, int img_width, float clip_thresh,
                   float* xys /*N*2*/, float* depths /*N*/, int* radii /*N*/, float* conics /*N*3*/,
                   float* compensation /*N*/, int* num_tiles_hit /*N*/, float* cov3d /*N*6*/,
                   int* tile_bounds /*N*4 or NULL*/, void* stream);
/* scratch of the ordered camera-gradient reduction of the three projection backwards below (P = 1 and with_touched = 0
 * for gs_project_bwd; with_touched = whether touched flags are passed) */
long long gs_project_pose_scratch_bytes(int N, int P, int with_touched);
/* v_viewmat[16] is accumulated into (caller zeroes; NULL to skip); v_depths / v_comp may be NULL. */
int gs_project_bwd(int N, const float* means3d, const float* scales, float glob_scale, const float* quats,
                   const float* viewmat, float fx, float fy, float cx, float cy, int img_height,
                   int img_width, float clip_thresh, const float* v_xys, const float* v_depths,
                   const float* v_conics, const float* v_comp, float* v_means3d, float* v_scales,
                   float* v_quats, float* v_viewmat,
                   int grad_flags /*bit 0: back-propagate through the fov clamp as if inactive, bit 1: quaternion gradient
                                    without the projection through q/|q| (gsplat 0.1.11's conventions);
                                    0 = the true derivatives*/,
                   void* pose_scratch /*with v_viewmat(s) / v_twist: gs_project_pose_scratch_bytes bytes, uninitialised — the
                                       camera-level gradients are summed over the Gaussians in a fixed order (block sums
                                       through one scratch row each, rows added in block order; round 6: they were fp32
                                       atomics whose order changed from run to run); NULL otherwise*/,
                         long long pose_scratch_bytes,
                         void* stream);

/* ---- gsplat.spherical_harmonics (upstream _C.compute_sh_forward/backward) ----
 * coeffs [N, K_stride, 3]; uses the first (degrees_to_use+1)^2 bases; dirs are normalised inside. */
int gs_sh_fwd(int N, int K_stride, int degrees_to_use, const float* viewdirs /*N*3*/,
              const float* coeffs, float* colors /*N*3*/, void* stream);
int gs_sh_bwd(int N, int K_stride, int degrees_to_use, const float* viewdirs, const float* v_colors,
              float* v_coeffs /*N*K_stride*3, fully written*/, void* stream);

/* ---- fused multi-sub-pose projection (the fork's per-sample loop in SplatfactoModel.get_outputs;
 * SURVEY §8 a2,a10; flags train.py:22,46,51,56,119).  Reads each Gaussian once, writes one record
 * per (sub-pose, Gaussian) with SH colour max(SH+0.5,0) and opacity*compensation. */
int gs_project_fused_fwd(int N, int P, const float* means3d, const float* scales, float glob_scale,
                         const float* quats, const float* opacities /*N, post-sigmoid*/,
                         const float* sh /*N*K_stride*3*/, int K_stride, int sh_degree,
                         const float* viewmats /*P*16*/, float fx, float fy, float cx, float cy,
                         int img_height, int img_width, float clip_thresh, int antialiased,
                         int defer_color /*bit 0: leave rgb = 0 and skip the SH read; gs_slice_colors fills it later.
                                           bit 1: write NO record for a culled (Gaussian, sub-pose) pair — its 64 bytes
                                           stay uninitialised; only for callers that never look at them (the sliced
                                           path behind gs_segmented_sort_compact_u32, which drops culled keys).
                                           bit 2 (round 5): band-aware — bits 8..23 hold R = rolling-shutter row bands;
                                           sub-pose p = s*R + r only composites tile rows [r*ty/R, (r+1)*ty/R): a pair
                                           whose tile box misses those rows is culled here (culled depth key, tile count
                                           0, no record), a box that straddles them is clipped to them.  `radii` keeps
                                           the un-banded value (the oracle's definition).
                                           bit 4 (round 5): write NO record at all (depth keys, tile counts and radii
                                           only): gs_frame_forward(desc->lazy_records) projects the records of the pairs
                                           its depth slices hold (gs_slice_project_records)*/,
                         float* records /*P*N*16*/, unsigned* depth_keys /*P*N*/,
                         int* num_tiles_hit /*P*N*/, int* radii /*P*N or NULL*/,
                         const float* sh_rest /*NULL, or features_rest [N*(K_stride-1)*3]: `sh` is then features_dc [N*3]
                                                (splatfacto keeps the two as separate parameters)*/,
                         int param_flags /*bit 0: `scales` holds LOG-scales (scale = exp), bit 1: `opacities` holds logits
                                           (opacity = sigmoid): the caller's raw parameters, no activation launches*/,
                         void* stream);
/* deferred SH colour of the slice Gaussians with counts[j] > 0 (global index slice_gi[j] = p*N + g) */
int gs_slice_colors(int n_slice, const unsigned* slice_gi, const unsigned* counts, int N, const float* means3d,
                    const float* sh, const float* sh_rest /*as in gs_project_fused_fwd*/, int K_stride, int sh_degree,
                    const float* viewmats, float* records, void* stream);
/* v_viewmats [P*16] accumulated into (caller zeroes; NULL to skip). */
int gs_project_fused_bwd(int N, int P, const float* means3d, const float* scales, float glob_scale,
                         const float* quats, const float* opacities, const float* sh, int K_stride,
                         int sh_degree, const float* viewmats, float fx, float fy, float cx, float cy,
                         int img_height, int img_width, float clip_thresh, int antialiased,
                         const float* records, const float* v_records, float* v_means3d, float* v_scales,
                         float* v_quats, float* v_opacities, float* v_sh, float* v_viewmats,
                         const unsigned char* touched /*[P*N] or NULL; 0 = that v_records row is zero and is not
                                                        read (set by gs_reduce_grad_tuples).  With touched given,
                                                        the caller must ZERO the five gradient outputs: Gaussians
                                                        untouched in every sub-pose are skipped entirely*/,
                         float* v_xy_sum /*[N*2] or NULL: sum over the sub-poses of the screen-space centre
                                           gradient (pixels) — the densification statistic splatfacto reads from
                                           xys.grad; same zeroing rule as the other outputs*/,
                         int grad_flags /*as in gs_project_bwd; + 8: skip the double-precision covariance chain that
                                          Gaussians with a scale ratio above 8 (needles) get by default; + 16
                                          (pixel-velocity model): v_records[.., 9..10] hold d loss / d pixel velocity
                                          from gs_rasterize_bwd_rs_slice; + 32 (needs touched): the kernel zero-fills the
                                          gradient outputs and v_xy_sum itself — hand over uninitialised buffers; + 64:
                                          v_records[.., 11] holds d loss / d camera-space depth (record float 9, from
                                          gs_frame_backward_depth) and is chained to the means and the view matrices
                                          (gs_project_pixvel_bwd: the mid-exposure view matrix only, no twist term);
                                          + 128 | (B << 8), B <= 256 dividing P (gs_project_fused_bwd, needs touched):
                                          v_xy_sum is [B,N,2] — row b = the sum over sub-poses [b*P/B, (b+1)*P/B)
                                          in sub-pose order, every row written (a frame of B cameras)*/,
                         const float* sh_rest, int param_flags /*both as in gs_project_fused_fwd: the gradients returned
                                          are those of what was handed in (d/d log-scale, d/d logit)*/,
                         float* v_sh_rest /*[N*(K_stride-1)*3] iff sh_rest != NULL (v_sh is then [N*3])*/,
                         void* pose_scratch /*with v_viewmat(s) / v_twist: gs_project_pose_scratch_bytes bytes, uninitialised — the
                                       camera-level gradients are summed over the Gaussians in a fixed order (block sums
                                       through one scratch row each, rows added in block order; round 6: they were fp32
                                       atomics whose order changed from run to run); NULL otherwise*/,
                         long long pose_scratch_bytes,
                         void* stream);
/* gs_project_fused_bwd on POOLED gradient buffers (grad flag 32 implied; bit-identical results).  The five (six)
 * gradient arrays are +0.0 everywhere except in the rows flagged in dirty[N] — what an earlier call on the same buffers
 * left behind (a fresh set: uninitialised arrays, dirty = all ones).  A block of the sparse kernel zeroes the dirty rows
 * of its 2048 Gaussians (more than a quarter of them dirty: it streams zeros over the whole chunk), writes this call's
 * rows and stores in `dirty` the map of them.  `touched`: the caller's persistent flag buffer — all zero before the frame
 * backward set this frame's flags, all zero again after this call (its last launch that reads the flags clears the ones
 * it found set).  v_viewmats [P*16] is STORED (uninitialised rows allowed, every float written).  The caller owns the
 * invariant: nothing else may have written to the arrays since the call that produced `dirty`. */
int gs_project_fused_bwd_pooled(int N, int P, const float* means3d, const float* scales, float glob_scale,
                                const float* quats, const float* opacities, const float* sh, int K_stride,
                                int sh_degree, const float* viewmats, float fx, float fy, float cx, float cy,
                                int img_height, int img_width, float clip_thresh, int antialiased,
                                const float* records, const float* v_records, float* v_means3d, float* v_scales,
                                float* v_quats, float* v_opacities, float* v_sh, float* v_viewmats,
                                unsigned char* touched, float* v_xy_sum, int grad_flags, const float* sh_rest,
                                int param_flags, float* v_sh_rest, void* pose_scratch, long long pose_scratch_bytes,
                                void* stream, unsigned char* dirty /*[N]*/);

/* ---- pixel-velocity model: the paper's first-order blur / rolling-shutter model (the fork's
 * own wording at /root/reference/README.md:200 "Fixed a bug in pixel velocity formulas").  ONE projection under the
 * mid-exposure `viewmat`; the record of sub-pose p is the same splat re-centred at xy + times[p] * pv with
 * pv = J * (-(ang x p_cam + lin)), J the pinhole Jacobian at the camera-space mean; conic, opacity, colour and the
 * depth key are shared by the P records (fixed depth order and covariance).  twist = {lin[3], ang[3]} (device,
 * OpenCV camera frame), times [P] (device, seconds).  Everything downstream (binning, compositor) is unchanged. */
int gs_project_pixvel_fwd(int N, int P, const float* means3d, const float* scales, float glob_scale,
                          const float* quats, const float* opacities, const float* sh, int K_stride, int sh_degree,
                          const float* viewmat /*16*/, const float* twist /*6*/, const float* times /*P*/,
                          float fx, float fy, float cx, float cy, int img_height, int img_width, float clip_thresh,
                          int antialiased, int defer_color, float* records, unsigned* depth_keys,
                          int* num_tiles_hit, int* radii, float rolling_shutter_time /*0: off.  != 0: EXACT per-row rolling shutter — sub-pose p is the blur
                                                        sample at times[p], the tile boxes are widened by the sweep
                                                        +- rolling_shutter_time / 2 * pixel velocity and the row term is
                                                        added by gs_rasterize_fwd_rs_slice / gs_rasterize_bwd_rs_slice*/,
                          float* pix_vel /*[N*2] out: pixel velocity of every Gaussian; NULL allowed when
                                           rolling_shutter_time == 0*/,
                          const float* sh_rest, int param_flags /*as in gs_project_fused_fwd*/, void* stream);
/* v_viewmat [16] and v_twist [12 floats: lin 3, ang 3, 6 unused] are accumulated into (caller zeroes; NULL skips) */
int gs_project_pixvel_bwd(int N, int P, const float* means3d, const float* scales, float glob_scale,
                          const float* quats, const float* opacities, const float* sh, int K_stride, int sh_degree,
                          const float* viewmat, const float* twist, const float* times, float fx, float fy,
                          float cx, float cy, int img_height, int img_width, float clip_thresh, int antialiased,
                          const float* records, const float* v_records, float* v_means3d, float* v_scales,
                          float* v_quats, float* v_opacities, float* v_sh, float* v_viewmat, float* v_twist,
                          const unsigned char* touched, float* v_xy_sum, int grad_flags, const float* sh_rest,
                          int param_flags, float* v_sh_rest /*as in gs_project_fused_bwd*/, void* pose_scratch /*with v_viewmat(s) / v_twist: gs_project_pose_scratch_bytes bytes, uninitialised — the
                                       camera-level gradients are summed over the Gaussians in a fixed order (block sums
                                       through one scratch row each, rows added in block order; round 6: they were fp32
                                       atomics whose order changed from run to run); NULL otherwise*/,
                         long long pose_scratch_bytes,
                         void* stream);

/* ---- gsplat-array <-> record glue for the rasterize_gaussians signature -------- */
int gs_pack_records(int N, const float* xys, const float* depths, const int* radii, const float* conics,
                    const float* colors /*N*3*/, const float* opacity /*N*/, int img_height, int img_width,
                    float* records /*N*16*/, unsigned* depth_keys /*N*/, int* num_tiles_hit /*N*/,
                    void* stream);
int gs_unpack_record_grads(int N, const float* v_records, float* v_xys, float* v_conics, float* v_colors,
                           float* v_opacity, void* stream);

/* ---- binning + sort (upstream map_gaussian_to_intersects, torch.sort, get_tile_bin_edges,
 * compute_cumulative_intersects) ------------------------------------------- */
long long gs_scan_workspace_bytes(long long n);
long long gs_radix_sort_workspace_bytes(long long n, int begin_bit, int end_bit);
/* exclusive prefix sum; *total_out (device, nullable) receives the grand total; in == out allowed */
int gs_exclusive_scan_u32(long long n, const unsigned* in, unsigned* out, unsigned* total_out, void* ws,
                          long long ws_bytes, void* stream);
/* stable LSD radix sort of (key, u32 value) pairs over key bits [begin_bit,end_bit); buffers 0 = input
 * (clobbered), buffers 1 = same-size scratch; *result_buf (HOST int) = which pair holds the result. */
int gs_radix_sort_pairs_u32(long long n, unsigned* keys0, unsigned* vals0, unsigned* keys1,
                            unsigned* vals1, int vals0_is_iota, int begin_bit, int end_bit, void* ws,
                            long long ws_bytes, int* result_buf /*host*/, void* stream);
/* gs_radix_sort_pairs_u32 whose FINAL pass also writes gather_out[i] = gather_src[value of sorted pair i]
 * (gather_out: n ints).  The tile sort of a depth slice sorts emission indices e and leaves the record index
 * gi_of_e[e] of every sorted entry for the scalar-cache compositors (gs_rasterize_*_slice: sorted_ids). */
int gs_radix_sort_pairs_gather_u32(long long n, unsigned* keys0, unsigned* vals0, unsigned* keys1, unsigned* vals1,
                                   int vals0_is_iota, int begin_bit, int end_bit, void* ws, long long ws_bytes,
                                   int* result_buf /*host*/, const unsigned* gather_src, unsigned* gather_out,
                                   const unsigned* n_dev /*NULL, or the real pair count on the device (n = capacity)*/,
                                   void* stream);
/* gs_radix_sort_pairs_u32 with a second payload per key: payload2_in[i] belongs to input element i (read only); the
 * passes ping-pong it through payload2_a / payload2_b (n ints each); *result_p2 (host) = 0 / 1: which of the two holds
 * it in sorted order.  Used by the tile sort of a depth slice (payload = emission index, payload 2 = record index). */
int gs_radix_sort_pairs_carry_u32(long long n, unsigned* keys0, unsigned* vals0, unsigned* keys1, unsigned* vals1,
                                  int vals0_is_iota, int begin_bit, int end_bit, void* ws, long long ws_bytes,
                                  int* result_buf /*host*/, const unsigned* payload2_in, unsigned* payload2_a,
                                  unsigned* payload2_b, int* result_p2 /*host*/,
                                  const unsigned* n_dev /*NULL, or the real pair count on the device*/, void* stream);
int gs_radix_sort_pairs_u64(long long n, unsigned long long* keys0, unsigned* vals0,
                            unsigned long long* keys1, unsigned* vals1, int vals0_is_iota, int begin_bit,
                            int end_bit, void* ws, long long ws_bytes, int* result_buf /*host*/,
                            void* stream);
/* segmented form: n = k*seg_len keys, each segment of seg_len keys sorted independently and stably by the
 * same launches (per-sub-pose depth pre-sort on 32-bit keys) */
long long gs_segmented_sort_workspace_bytes(long long n, long long seg_len, int begin_bit, int end_bit);
int gs_segmented_sort_pairs_u32(long long n, long long seg_len, unsigned* keys0, unsigned* vals0,
                                unsigned* keys1, unsigned* vals1, int vals0_is_iota, int begin_bit, int end_bit,
                                void* ws, long long ws_bytes, int* result_buf /*host*/, void* stream);
/* compacting form (the depth pre-sort of the sliced path): keys equal to skip_key — culled Gaussians — are dropped
 * by the first pass; segment s ends up with its seg_counts[s] (device) surviving keys sorted at
 * [s*seg_len, s*seg_len + seg_counts[s]), the rest of the segment is unspecified.  Payload = global index.
 * gather_src/gather_out (NULL together): gather_out[slot] = gather_src[payload] of every sorted survivor. */
long long gs_segmented_sort_compact_workspace_bytes(long long n, long long seg_len, int begin_bit, int end_bit,
                                                    int max_digit_bits);
int gs_segmented_sort_compact_u32(long long n, long long seg_len, unsigned* keys0, unsigned* vals0,
                                  unsigned* keys1, unsigned* vals1, int begin_bit, int end_bit,
                                  int max_digit_bits /*8..11: widest radix digit (fewest passes of equal width)*/,
                                  unsigned skip_key,
                                  unsigned* seg_counts /*device, n/seg_len*/, const unsigned* gather_src,
                                  unsigned* gather_out, void* ws, long long ws_bytes, int* result_buf /*host*/,
                                  void* stream);
/* ---- nearest-first selection (round 6; MI355X design, no upstream counterpart: upstream sorts every intersection,
 * SURVEY.md §8 a5) -----------------------------------------------------------------------------------------------
 * A frame whose tiles saturate early composites a few percent of its visible (sub-pose, Gaussian) pairs.  Instead of
 * ordering all of them, gs_depth_select finds per segment (sub-pose) the key bound below which the pairs carry `budget`
 * of the weights (their bounding-box tile counts), two histogram launches over key bits 30..20 and 19..9;
 * gs_segmented_sort_select_u32 then keeps and sorts only the keys inside a per-segment range — [0, bound) for the first
 * depth slice, [bound, culled) for the rest, if the frame turns out to need it (gs_frame_forward, depth_select). */
long long gs_depth_select_workspace_bytes(int segments);
/* thr_out[s] = smallest multiple of 512 with: weight of the keys < thr_out[s] of segment s >= budget (0x80000000: the
 * whole segment carries less).  Keys with bit 31 set are culled pairs.  *grand_out (device u32, nullable) += weight of
 * every visible pair.  ws (gs_depth_select_workspace_bytes) and *grand_out must be ZERO on entry. */
int gs_depth_select(long long n, long long seg_len, const unsigned* keys, const unsigned* weights, long long budget,
                    unsigned* thr_out /*device, n/seg_len*/, unsigned* grand_out, void* ws, long long ws_bytes,
                    void* stream);
/* gs_segmented_sort_compact_u32 over the keys inside [key_lo[s], key_hi[s]) only (device arrays per segment, either
 * NULL = unbounded; skip_key is dropped as well).  keys_src is read by the first pass and left INTACT, keys0 / keys1 are
 * scratch of n keys each; workspace as gs_segmented_sort_compact_workspace_bytes. */
int gs_segmented_sort_select_u32(long long n, long long seg_len, const unsigned* keys_src, unsigned* keys0,
                                 unsigned* vals0, unsigned* keys1, unsigned* vals1, int begin_bit, int end_bit,
                                 int max_digit_bits, unsigned skip_key, const unsigned* key_lo, const unsigned* key_hi,
                                 unsigned* seg_counts, const unsigned* gather_src, unsigned* gather_out, void* ws,
                                 long long ws_bytes, int* result_buf /*host*/,
                                 long long tail_cap /*0, or a PROMISE that no segment keeps more keys than this: the
                                                     passes behind the compacting one are sized for it; a segment that
                                                     keeps more comes out wrong — check seg_counts*/,
                                 void* stream);
/* exclusive scan where only the first seg_counts[s] values of every seg_len-long segment are live (the rest count as
 * zero and are never read).  out is defined for the live ranks and at every segment's first rank (the slice plan reads
 * those); behind a segment's live ranks it is unspecified */
int gs_exclusive_scan_segments_u32(long long n, long long seg_len, const unsigned* seg_counts /*device*/,
                                   const unsigned* in, unsigned* out, unsigned* total_out /*device, 1*/, void* ws,
                                   long long ws_bytes, void* stream);
/* out[i] = (i / N) << 32 | depth_keys[i] : the (sub-pose, depth) key of the N-sized pre-sort (64-bit route) */
int gs_make_depth_keys64(long long n, int N, const unsigned* depth_keys, unsigned long long* out,
                         void* stream);
int gs_gather_counts(long long n, const unsigned* sorted_gi, const int* num_tiles_hit,
                     unsigned* counts_out, void* stream);
/* keys[e] = p*T + tile, vals[e] = p*N + g, emitted in depth-rank order.  invalid_key != 0 enables exact
 * tile culling: a (Gaussian, tile) pair whose pixel-centre rectangle lies outside the alpha >= 1/255
 * ellipse gets key = invalid_key (pass S*R*T: it sorts behind every real tile and is never composited) */
int gs_emit_intersects(long long n_ranked, int N, int img_height, int img_width, const unsigned* sorted_gi,
                       const unsigned* cum_excl, const float* records, long long n_isect, unsigned* keys,
                       unsigned* vals, unsigned invalid_key, void* stream);
int gs_tile_bin_edges_u32(long long n, const unsigned* sorted_keys, int num_bins, int* bins /*num_bins*2*/,
                          const unsigned* n_dev /*NULL, or the real entry count on the DEVICE (n is then the capacity
                                                  the launch is sized for): no host read-back of a slice's size*/,
                          void* stream);
int gs_tile_bin_edges_u64(long long n, const unsigned long long* sorted_isect_ids, int num_bins,
                          int* bins /*num_bins*2*/, void* stream);
/* gs_tile_bin_edges_u32 fused with the gather ids_out[i] = gi_of_e[sorted_vals[i]] (i < n), ids_out[n..n+8) = 0:
 * the record index of every sorted entry of a depth slice, read by the compositors through the scalar cache */
int gs_tile_bin_edges_ids_u32(long long n, const unsigned* sorted_keys, int num_bins, int* bins /*num_bins*2*/,
                              const unsigned* sorted_vals, const unsigned* gi_of_e, unsigned* ids_out /*n+8*/,
                              void* stream);
/* upstream-format ids: isect_id = tile<<32 | float_bits(depth); cum_tiles_hit is the INCLUSIVE cumsum */
int gs_map_gaussian_to_intersects(int N, const float* xys, const float* depths, const int* radii,
                                  const int* cum_tiles_hit, int img_height, int img_width,
                                  long long* isect_ids, int* gaussian_ids, void* stream);

/* ---- gsplat.rasterize_gaussians (upstream _C.rasterize_forward / rasterize_backward; SURVEY §8
 * a7,a8).  S sample images x R rolling-shutter row bands: sub-pose p = s*R + r renders tile rows
 * [band_edges[r], band_edges[r+1]) of sample s.  tile_bins is [S*R*T, 2]. */
int gs_rasterize_fwd(const float* records, const int* sorted_vals, const int* tile_bins,
                     const int* band_edges /*R+1*/, const float* background /*3*/, int S, int R,
                     int img_height, int img_width, float* out_img /*S*H*W*3*/, float* out_T /*S*H*W*/,
                     int* final_idx /*S*H*W*/,
                     int n_records /*rows of `records`.  > 0 selects the scalar-cache compositor (variant 0), which
                                     reads sorted_vals in aligned groups of four: the array must then have 8 readable
                                     ints past its last entry (values are clamped to n_records-1, never blended)*/,
                     int variant /*0.  (1, 2: the round-1 v_readlane compositors — compiled only into the test library
                                   tests/libgsdeblur_round1.so, -DGS_ROUND1_KERNELS=1; the product returns GS_ERR_INVALID)*/,
                     void* stream);
/* v_records [P*N*12] is accumulated into with fp32 atomics (caller zeroes); v_alpha may be NULL. */
int gs_rasterize_bwd(const float* records, const int* sorted_vals, const int* tile_bins,
                     const int* band_edges, const float* background, int S, int R, int img_height,
                     int img_width, const float* out_T, const int* final_idx, const float* v_img,
                     const float* v_alpha, float* v_records,
                     int n_records /*as in gs_rasterize_fwd: > 0 selects the scalar-cache kernel (padded sorted_vals)*/,
                     int variant /*0 (2: the round-1 kernel, test library only, see gs_rasterize_fwd); + 256: let the
                                   gradient pass the alpha = min(0.999, .) clamp as gsplat 0.1.11 does*/,
                     void* stream);

/* ---- depth-sliced variant of the same path (MI355X design, no upstream counterpart) ----------
 * With early termination only a few percent of the (Gaussian, tile) intersections are ever
 * composited.  The depth-ranked Gaussians are processed in front-to-back slices; a tile whose
 * pixels have all stopped is flagged done and later slices emit no intersections for it.  Every
 * pixel still sees the same Gaussians in the same order, so results equal the unsliced pass. */
/* bounds[p*K+k] = first depth rank of sub-pose p whose cumulative intersection count reaches base<<k;
 * rels[p*K+k] = that cumulative count at the boundary (sub-pose total when the boundary is N — which the LAST
 * boundary need not be: read the totals from seg_totals) */
int gs_slice_plan(int P, int N, int K, const unsigned* cum_excl /*P*N, rank order*/,
                  const unsigned* total /*device: grand total of the scan*/, long long base,
                  int* bounds /*P*K*/, unsigned* rels /*P*K*/,
                  unsigned* seg_totals /*P or NULL: every sub-pose's own intersection total (mod 2^32)*/,
                  const unsigned* n_live /*P or NULL: ranks [n_live[p], N) of sub-pose p hold nothing (compacting
                                           pre-sort); boundaries then never exceed n_live[p]*/,
                  unsigned* tail /*NULL, or P+1: receives the live rank count of every sub-pose (N without n_live) and
                                   then the grand total — so that one device->host copy of a buffer holding bounds,
                                   rels, seg_totals and tail back to back brings the whole plan over*/,
                  void* stream);
/* gs_slice_plan when the ranked pairs are a nearest-first selection: every boundary lies behind them (one slice holds
 * the whole selection) and tail[P] = *grand (device: gs_depth_select's grand_out), the frame's total over ALL pairs */
int gs_slice_plan_select(int P, int N, int K, const unsigned* cum_excl, const unsigned* total, int* bounds,
                         unsigned* rels, unsigned* seg_totals, const unsigned* n_live, unsigned* tail,
                         const unsigned* grand, void* stream);
/* sat [P*(tiles_y+1)*(tiles_x+1)] = summed-area table of tiles NOT done (tile_done u8 [P*T]) */
int gs_tile_open_sat(int P, int img_height, int img_width, const unsigned char* tile_done, int* sat,
                     unsigned long long* open_bits /*NULL or [P*tiles_y*ceil(tiles_x/64)]: bit x of row y set while
                                                     tile (x, y) is open (consumed by gs_slice_counts_exact)*/,
                     const int* gate /*NULL, or the open_flag word of the previous slice's forward compositor: 0 there
                                       = no tile is open, the launch does nothing*/,
                     void* stream);
/* slice = for each sub-pose p the depth ranks sorted_gi[slice_begin[p] + i], i < prefix[p+1]-prefix[p]
 * (slice_begin / slice_prefix are HOST arrays, P <= 256: they travel in the kernel arguments);
 * writes slice_gi[j] (global index) and counts[j] (open tiles; sat == NULL: all tiles open) */
int gs_slice_counts(int n_slice, int P, int N, const int* slice_begin /*P, HOST*/, const int* slice_prefix /*P+1, HOST*/,
                    const unsigned* sorted_gi, const float* records, const int* sat, int img_height,
                    int img_width, unsigned* slice_gi, unsigned* counts, void* stream);
/* exact counts: tiles of the box that are open AND pass the ellipse test of gs_emit_*; with these counts and
 * compact != 0 the emission holds no culled pairs at all (sat / tile_done NULL: every tile is open) */
int gs_slice_counts_exact(int n_slice, int P, int N, const int* slice_begin /*HOST*/, const int* slice_prefix /*HOST*/,
                          const unsigned* sorted_gi, const float* records, const int* sat,
                          const unsigned char* tile_done, int img_height, int img_width, unsigned* slice_gi,
                          unsigned* counts, int wave_per_gaussian /*1: one Gaussian per wave (few, large boxes)*/,
                          const unsigned* cum_rank /*[P*N] exclusive prefix of num_tiles_hit in depth-rank order (the
                                                     array gs_slice_plan reads); needed with hit_masks*/,
                          unsigned long long* hit_masks /*NULL, or >= total/64 + n_slice + 1 words: one bit per box
                                                          tile (open AND inside the ellipse) for gs_emit_open_intersects;
                                                          requires the u32 prefix not to have wrapped (total < 2^32)*/,
                          unsigned* mask_off /*[n_slice] first mask word of each slice Gaussian, or NULL*/,
                          const unsigned long long* open_bits /*from gs_tile_open_sat; NULL exactly when tile_done is*/,
                          const int* gate /*NULL, or the previous slice's open_flag word (device): 0 there = every
                                            count is 0 without looking at anything — a slice launched before anybody
                                            knows whether it is needed costs next to nothing when it is not*/,
                          void* stream);
/* gs_slice_counts_exact for the lists of the pixel-velocity compositors (round 6): the alpha >= 1/255 ellipse swept
 * over the times a tile row's pixels can see the splat — sample times in [t_min, t_max] (0, 0 for per-sample lists)
 * plus the row time ((y + 0.5) / H - 0.5) * rolling_shutter_time — centre = records[gi].xy + t * pix_vel[gi % N].
 * hit_masks / cum_rank / mask_off are required (the emission expands the masks); no upstream counterpart (upstream
 * lists hold whole bounding boxes). */
int gs_slice_counts_exact_swept(int n_slice, int P, int N, const int* slice_begin, const int* slice_prefix,
                                const unsigned* sorted_gi, const float* records, const int* sat,
                                const unsigned char* tile_done, int img_height, int img_width, unsigned* slice_gi,
                                unsigned* counts, int wave_per_gaussian, const unsigned* cum_rank,
                                unsigned long long* hit_masks, unsigned* mask_off, const unsigned long long* open_bits,
                                const float* pix_vel, float t_min, float t_max, float rolling_shutter_time,
                                void* stream);
int gs_emit_open_intersects(int n_slice, int N, int img_height, int img_width, const unsigned* slice_gi,
                            const unsigned* counts, const unsigned* cum_excl, const float* records,
                            const unsigned char* tile_done /*NULL: all open*/, unsigned* keys, unsigned* vals,
                            unsigned invalid_key, int compact /*1: counts are exact, culled pairs take no slot*/,
                            int wave_per_gaussian,
                            const unsigned long long* hit_masks /*from gs_slice_counts_exact, or NULL: redo the tests*/,
                            const unsigned* mask_off,
                            unsigned char* tile_hot /*NULL, or [S*R*T] zeroed by the caller: set to 1 for every tile that
                                                      receives a Gaussian whose opacity exceeds the 0.999 alpha clamp;
                                                      the compositors run their clamp-free loop on the other tiles*/,
                            void* stream);
/* one launch per slice, front to back; out_img/out_T/live_T carry per-pixel state, tile_done is zeroed
 * by the caller before the first slice; first && last == the unsliced pass; final_idx is per slice */
int gs_rasterize_fwd_slice(const float* records, const int* sorted_vals, const int* tile_bins,
                           const int* band_edges, const float* background, int S, int R, int img_height,
                           int img_width, float* out_img, float* out_T, float* live_T, int* final_idx,
                           unsigned char* tile_done, int first, int last,
                           const int* gi_of_e /*NULL: sorted_vals are Gaussian ids; else sorted_vals are emission
                                                indices e and the Gaussian id is gi_of_e[e]*/,
                           const int* sorted_ids /*[I+8] record index of every sorted entry (gs_tile_bin_edges_ids_u32),
                                                   or NULL: taken from sorted_vals when gi_of_e is NULL (padded as in
                                                   gs_rasterize_fwd), else the v_readlane compositor runs*/,
                           int n_records /*rows of `records`; <= 0 forces the v_readlane compositor*/,
                           float* out_depth /*[S*H*W] or NULL: sum over the blended entries of weight * camera-space
                                              depth (record float 9), carried between slices like out_img; expected
                                              depth = this / alpha — what splatfacto returns as outputs["depth"]
                                              (/root/reference/render_model.py:219).  Scalar-cache compositor only*/,
                           const unsigned char* tile_hot /*from gs_emit_open_intersects for THIS slice, or NULL: every
                                                           tile runs the loop with the alpha clamp*/,
                           int* open_flag /*NULL, or one int zeroed by the caller: receives the number of tiles still
                                            open after this slice (last == 0 only)*/,
                           int variant /*0 (1, 2: the round-1 v_readlane compositor, test library only, see
                                         gs_rasterize_fwd; the lock-step walk of round 3, variant 3, was removed)*/,
                           void* stream);
/* Debug twin of gs_rasterize_fwd_slice (no upstream counterpart; DESIGN.md section 5 "lane utilisation"): same outputs
 * through the round-1 compositor, and the counters of its walk summed into stats[13] (u64, zeroed by the caller):
 * [0] list entries walked, [1] pixels blended (hit and live), [2] pixels with alpha >= 1/255 (live or not), [3]/[4] 4x4
 * pixel blocks / 8x8 quadrants with such a pixel, [5]/[6] steps a 64-entry chunk would take if every block / quadrant
 * walked only its own entries in lock-step, [7] chunks, [8] entries with a live hit, [9]/[10] blocks / quadrants with a
 * live hit, [11]/[12] as [5]/[6] for live hits. */
int gs_rasterize_fwd_slice_stats(const float* records, const int* sorted_vals, const int* tile_bins,
                                 const int* band_edges, const float* background, int S, int R, int img_height,
                                 int img_width, float* out_img, float* out_T, float* live_T, int* final_idx,
                                 unsigned char* tile_done, int first, int last, const int* gi_of_e, int* open_flag,
                                 unsigned long long* stats, void* stream);
/* ---- exact per-row rolling shutter of the pixel-velocity model (csrc/raster_rs.hip; SURVEY App. A "Paper's blur/RS
 * model", flag /root/reference/train.py:56, field /root/reference/render_video.py:242-243).  ONE record per (blur
 * sample, Gaussian); pixel row y evaluates the splat at xy + tau(y) * pix_vel[g], tau(y) = ((y + 0.5)/H - 0.5) * T_ro.
 * Same slice / state protocol as gs_rasterize_fwd_slice / gs_rasterize_bwd_slice with R = 1; sorted_ids [I+8] is the
 * record index of every sorted entry, sorted_vals its emission index (tuple slot).  The backward's tuples carry
 * d loss / d pix_vel in slots 9 and 10 (gs_reduce_grad_tuples sums them into v_records[.., 9..10];
 * gs_project_pixvel_bwd picks them up with grad_flags + 16). */
int gs_rasterize_fwd_rs_slice(const float* records, const int* tile_bins, const int* band_edges, const float* background,
                              int S, int img_height, int img_width, float* out_img, float* out_T, float* live_T,
                              int* final_idx, unsigned char* tile_done, int first, int last, const int* sorted_ids,
                              int n_records, float* out_depth, int* open_flag, const float* pix_vel, int N,
                              float rolling_shutter_time,
                              const float* shared_list_times /*NULL, or [S] (device): ONE record set / tile list (that of
                                 sub-pose 0: records [N], tile_bins [T]) for all S samples; sample s evaluates every splat
                                 at xy + (shared_list_times[s] + tau(y)) * pix_vel[g].  tile_done stays [S*T]*/,
                              void* stream);
int gs_rasterize_bwd_rs_slice(const float* records, const int* sorted_vals, const int* tile_bins, const int* band_edges,
                              const float* background, int S, int img_height, int img_width, const float* out_T,
                              const int* final_idx, const float* v_img, const float* v_alpha, float* bwd_T, float* bwd_B,
                              float* tuples, unsigned char* flags, const int* sorted_ids, int n_records, int variant,
                              const float* cmb_scale, float cmb_gamma, float cmb_min_level, const float* pix_vel, int N,
                              float rolling_shutter_time,
                              const float* shared_list_times /*as in the forward; then tuples [I*S*12] / flags [I*S]: the
                                 gradients of entry e from sample s land in tuple e*S + s (gs_reduce_grad_tuples with
                                 tuples_per_entry = S)*/,
                              void* stream);
/* one launch per slice, back to front; bwd_T (init = out_T) and bwd_B [S,H,W] (behind-colour . v_out, init = 0)
 * carry the reverse-traversal state; both may be NULL on the tuple path when the frame has a single slice */
int gs_rasterize_bwd_slice(const float* records, const int* sorted_vals, const int* tile_bins,
                           const int* band_edges, const float* background, int S, int R, int img_height,
                           int img_width, const float* out_T, const int* final_idx, const float* v_img,
                           const float* v_alpha, float* bwd_T, float* bwd_B, float* v_records,
                           const int* gi_of_e /*as in the forward*/,
                           float* tuples /*[I*12] or NULL*/, unsigned char* flags /*[I], zeroed, or NULL*/,
                           const int* sorted_ids /*as in gs_rasterize_fwd_slice*/, int n_records,
                           const unsigned char* tile_hot /*as in gs_rasterize_fwd_slice (same slice)*/,
                           int variant /*0 (2: round-1 kernel, test library only); + 256: upstream alpha-clamp
                                         gradient, as in gs_rasterize_bwd; + GS_BWD_ABSGRAD (tuple form only): tuple
                                         slots 9 and 10 of every flagged tuple receive the entry's absgrad sums*/,
                           const float* cmb_scale /*[H,W,3] or NULL.  Non-NULL folds gs_combine_bwd into this launch:
                                                    v_img then holds the SAMPLE IMAGES [S,H,W,3] and each pixel derives
                                                    its sample gradient from cmb_scale (gs_combine_bwd_scale)*/,
                           float cmb_gamma, float cmb_min_level, void* stream);

/* Atomic-free gradient accumulation: with gi_of_e, tuples and flags given, gs_rasterize_bwd_slice writes the 9
 * gradients of sorted entry i to tuples[e*12..] (e = sorted_vals[i]) and sets flags[e]; the tuples of slice
 * Gaussian j are the contiguous range [cum_excl[j], cum_excl[j]+counts[j]) and this call sums them into
 * v_records[slice_gi[j]] with plain stores (each Gaussian belongs to exactly one slice). */
int gs_reduce_grad_tuples(int n_slice, const unsigned* slice_gi, const unsigned* counts,
                          const unsigned* cum_excl, const float* tuples, const unsigned char* flags,
                          float* v_records, unsigned char* touched /*[P*N] or NULL: set to 1 where written*/,
                          long long n_isect /*entries of the slice: picks the kernel form*/,
                          const float* records /*[P*N,16]: flags[e] == 2 (tuples of the scalar-cache kernel) marks slot 5
                                                 as the plain sum of v_sigma; the reduce divides it by -opacity*/,
                          int tuples_per_entry /*1; S for gs_rasterize_bwd_rs_slice with one list for S samples: entry e's
                                                 tuples are e*S .. e*S+S-1*/,
                          void* stream);

/* ---- sub-frame averaging in linearised colour (flags train.py:60,62) ---------
 * out = ( mean_k max(C_k, min_level)^gamma )^(1/gamma); n = H*W*3 values per sample. */
int gs_combine_fwd(int S, long long n, const float* samples /*S*n*/, float gamma, float min_level,
                   float* out /*n*/, void* stream);
int gs_combine_bwd(int S, long long n, const float* samples, float gamma, float min_level,
                   const float* out, const float* v_out, float* v_samples /*S*n*/, void* stream);
/* the sample-independent factor of gs_combine_bwd: scale[i] = (1/S) * out[i]^(1-gamma)/gamma * v_out[i] */
int gs_combine_bwd_scale(int S, long long n, float gamma, const float* out, const float* v_out,
                         float* scale /*n*/, void* stream);
/* the three calls above for B cameras in ONE launch: samples / v_samples [B*S*n] (camera b's S sample images
 * contiguous), out / v_out / scale [B*n]; camera b's rows are bit-identical to the single-camera call on its slice */
int gs_combine_fwd_batched(int B, int S, long long n, const float* samples, float gamma, float min_level,
                           float* out, void* stream);
int gs_combine_bwd_batched(int B, int S, long long n, const float* samples, float gamma, float min_level,
                           const float* out, const float* v_out, float* v_samples, void* stream);
int gs_combine_bwd_scale_batched(int B, int S, long long n, float gamma, const float* out, const float* v_out,
                                 float* scale, void* stream);

/* ---- data-parallel gradient exchange (no reference counterpart: the reference is single-GPU,
 *      train.py:114-122 passes no device / world-size flags) -------------------------------------------------
 * The Gaussian gradient tensors share the leading dimension N; tensor t has widths[t] floats per row
 * (means 3, scales 3, quats 4, opacities 1, features_dc 3, features_rest 45 at SH degree 3; a tensor of width 0 —
 * features_rest at degree 0 — takes no payload column and its pointer may be null).  `grads` and
 * `widths` are HOST arrays of n_tensors (<= 16) entries; grads[t] are device pointers.
 * A payload row is wtot = sum(widths) floats followed by the row index as an int32 bit pattern. */
int gs_dp_row_mask(int N, int n_tensors, float* const* grads, const int* widths,
                   unsigned char* mask /*N: 1 where any of the row's floats is non-zero*/, void* stream);
int gs_dp_pack_rows(long long M, const long long* row_idx /*M, device, int64*/, int n_tensors,
                    float* const* grads, const int* widths, float* payload /*M*(wtot+1)*/, void* stream);
/* grads[t][row] += scale * payload row, for the M payload rows; the row indices of ONE payload must be unique
 * (no atomics).  Apply the ranks' payloads in rank order for a bit-identical sum on every rank. */
int gs_dp_scatter_add_rows(long long M, const float* payload, int n_tensors, float* const* grads,
                           const int* widths, float scale, void* stream);
/* Fixed-capacity, sync-free form of the same exchange (no row count ever reaches the host): payload is
 * [(cap+1)*(wtot+1)] floats, row 0 a header of int bit patterns {rows with a gradient on the sender, rows packed =
 * min(that, cap)}, rows 1.. the packed rows.  pos = exclusive prefix sum of mask (int32 [N]); idx_ws: cap ints. */
int gs_dp_pack_masked_rows(int N, const unsigned char* mask, const int* pos, int cap, int* idx_ws, int n_tensors,
                           float* const* grads, const int* widths, float* payload, void* stream);
int gs_dp_scatter_add_payload(int cap, const float* payload, int n_tensors, float* const* grads, const int* widths,
                              float scale, void* stream);

/* ---- lazy records (round 5) ---------------------------------------------------------------------------------------
 * A frame projected with gs_project_fused_fwd(defer_color bit 4) has depth keys, tile counts and radii but NO records;
 * the records of the (sub-pose, Gaussian) pairs a depth slice holds are projected when the slice is issued, by the same
 * arithmetic (bit-identical rows).  `gs_project_inputs` = the arguments of that gs_project_fused_fwd call. */
typedef struct gs_project_inputs {
  const float *means, *scales, *quats, *opacities, *viewmats;   /* as gs_project_fused_fwd (viewmats [P*16]) */
  float glob_scale, fx, fy, cx, cy, clip_thresh;
  int antialiased, defer_color, param_flags;
} gs_project_inputs;
/* slice_begin / slice_prefix / sorted_gi: as gs_slice_counts_exact; records [P*N*16] */
int gs_slice_project_records(int n_slice, int P, int N, const int* slice_begin, const int* slice_prefix,
                             const unsigned* sorted_gi, const gs_project_inputs* in, int img_height, int img_width,
                             float* records, void* stream);
/* the records of ALL pairs of such a frame in one coalesced pass (nothing but records is written); gs_frame_forward calls
 * it once when a lazy frame goes beyond its first depth slice */
int gs_project_records(int P, int N, const struct gs_project_inputs* in, int img_height, int img_width, float* records,
                       void* stream);

/* ---- one frame's depth-sliced pipeline issued by the library itself (csrc/frame.hip) -------------------------------
 * What the fork's Python layer does between project_gaussians and the returned image — binning, sorting and compositing
 * (boundary §8b: "caller owns all tensors; the library allocates nothing; workspace passed in") — as
 * TWO calls instead of ~45 per frame from the host language: every buffer comes out of ONE caller-owned arena (bump
 * allocation), the slice plan and one word per depth slice come back through caller-owned pinned host memory, and the
 * backward walks the slice table the forward leaves in *state (a plain host struct; byte offsets into the arena). */
#define GS_FRAME_MAX_SLICES 16
typedef struct gs_frame_desc {
  int N, P, S, R, H, W;      /* Gaussians, sub-poses (= S*R), sample images, rolling-shutter bands, image size */
  int slice_base;            /* average tile-list budget of the first depth slice (doubles per slice); 0: one slice */
  int depth_sort_digit;      /* widest radix digit of the depth pre-sort (8..11) */
  int fwd_variant;           /* as gs_rasterize_fwd_slice: 0 */
  int reserve_backward;      /* 1: the arena must also hold what gs_frame_backward will take */
  float merge_open_fraction; /* > 0: a slice that leaves at least this fraction of its open tiles open makes the next
                                issued slice span twice as many planned ones (frames whose tiles do not saturate gain
                                nothing from slice boundaries); 0: every planned slice is issued on its own */
  float rolling_shutter_time;/* != 0 (with pix_vel != NULL, R == 1): exact per-row rolling shutter of the pixel-velocity
                                model — box lists + the gs_rasterize_*_rs_slice compositors */
  int poll_readback;         /* 1: the plan and the open-tile count reach the host through a one-block kernel that
                                writes into host_pinned and a sequence word the host polls (no stream synchronisation
                                per read-back); 0: hipMemcpyAsync + hipStreamSynchronize */
  int shared_list;           /* 1 (pixel-velocity model, P == 1, R == 1, pix_vel and sample_times given): ONE record set
                                (the mid-exposure splats, tile boxes swept over exposure + readout), ONE depth sort and ONE
                                tile list for all S blur samples — the paper's form (depth order and covariance fixed
                                across samples; SURVEY.md App. A, /root/reference/README.md:196-200); sample s evaluates
                                every splat at mu' + (sample_times[s] + tau(y)) * pixel velocity inside the compositor */
  float combine_gamma;       /* with out_combined != NULL: gs_combine_fwd(gamma, min_level) of the sample images is */
  float combine_min_level;   /* launched behind every slice's compositor (it overlaps the open-tile read-back) */
  int band_clipped;          /* 1: the projection was band-aware (gs_project_fused_fwd defer_color bit 2): a sub-pose's
                                tile counts only hold the pairs inside its rolling-shutter band, so a sub-pose owns T/R
                                open tiles and the slice plan's budget per sub-pose is T/R * slice_base (0: T * slice_base,
                                of which one pair in R lies inside the band) */
  int depth_select;          /* 1 (with slice_base > 0): nearest-first selection — the depth pre-sort only ranks the pairs
                                the first slice's budget reaches (gs_depth_select + gs_segmented_sort_select_u32); the
                                pairs behind them are sorted and planned (budget doubled) only if that slice leaves a
                                tile open.  Same images bit for bit; for scenes whose frames stop in their first slice */
  int select_cap;            /* depth_select: 0, or a bound on the pairs a sub-pose's selection holds (what the last frame's did,
                                with slack): the sort passes over the selection are sized for it instead of for N.  Checked
                                — a frame that selects more sorts again without it (gs_frame_state.select_overflow) */
  float sweep_t_min, sweep_t_max; /* shared_list: smallest / largest of sample_times (host copies): with planned slices the
                                lists are culled by the alpha >= 1/255 ellipse swept over [sweep_t_min, sweep_t_max] + the
                                row times (gs_slice_counts_exact_swept) instead of holding the swept boxes whole */
  const struct gs_project_inputs* lazy_records;   /* NULL, or (the projection ran with defer_color bit 4: `records` holds
                                nothing yet) what it was called with: every issued slice first projects the records of
                                its own pairs (gs_slice_project_records).  SE(3) sub-poses only (pix_vel == NULL) */
  int cameras;               /* 0 or 1: one camera.  B > 1 (SE(3) sub-poses, B divides S): the frame holds B cameras —
                                camera b owns sample images [b*S/B, (b+1)*S/B) and sub-poses [b*P/B, (b+1)*P/B), S stays
                                the number of sample images; out_combined is then [B,H,W,3] (gs_combine_fwd_batched) and
                                the backward's cmb_scale [B,H,W,3] (gs_combine_bwd_scale_batched).  The 32-bit pixel
                                offsets keep S*H*W < 2^30 for the whole batch */
} gs_frame_desc;
typedef struct gs_frame_slice {
  long long I;               /* capacity of the slice's lists (its ranks' bounding-box pairs); real count on the device */
  int n, wave_per_gaussian, first, last;
  long long svals, bins, fidx, gi_of_e, sorted_ids, slice_gi, counts, cum, tile_hot, n_emitted_dev;   /* arena offsets */
} gs_frame_slice;
typedef struct gs_frame_state {
  int n_slices, P, N, S, R, H, W;
  float rolling_shutter_time;/* copied from the descriptor (0: not an exact-rolling-shutter frame) */
  int shared_list;           /* copied from the descriptor */
  int depth_select;          /* 0: every visible pair was depth-sorted; 1: only the nearest-first selection; 2: the
                                selection, and later the pairs behind it (the first slice left tiles open) */
  int select_overflow;       /* 1: the selection outgrew desc.select_cap and was sorted a second time */
  float open_after_first;    /* share of the (sample, tile) lists the frame's FIRST issued slice left open (its read-back:
                                0 = every tile stopped within it); -1: the first slice was also the last, nothing was read */
  long long n_total;         /* bounding-box tile intersections of the frame */
  long long max_selected;    /* depth_select: the most pairs any sub-pose's selection held (0 otherwise) */
  long long arena_used;      /* bytes of the arena the forward occupies (kept alive until the backward ran) */
  long long arena_required;  /* on GS_ERR_WORKSPACE (3): an arena size that holds the frame as far as it is known */
  gs_frame_slice slice[GS_FRAME_MAX_SLICES];
  int cameras;               /* copied from the descriptor (1 for 0) */
} gs_frame_state;
/* records / depth_keys (consumed) / num_tiles_hit: outputs of gs_project_fused_fwd or gs_project_pixvel_fwd;
 * band_tile_done [P*T] u8: initial done mask of a rolling-shutter frame (R > 1; NULL otherwise); color_*: deferred SH
 * colour inputs (all NULL: records already hold colours); out_depth nullable [S*H*W] (zeroed by the caller);
 * host_pinned: >= 4*(2*P*16 + 2*P + 2) + 64 bytes of pinned, device-visible host memory (hipHostMalloc / torch pin_memory).  On GS_ERR_WORKSPACE call again with a larger
 * arena AND fresh projection outputs (depth_keys was consumed). */
int gs_frame_forward(const gs_frame_desc* desc, float* records, unsigned* depth_keys, const int* num_tiles_hit,
                     const float* background /*3*/, const int* band_edges /*R+1*/, const unsigned char* band_tile_done,
                     const float* color_means, const float* color_sh, const float* color_sh_rest /*as sh_rest of
                     gs_project_fused_fwd*/, int color_K_stride, int color_sh_degree,
                     const float* color_viewmats /*P*16*/,
                     const float* pix_vel /*NULL, or [N*2] from gs_project_pixvel_fwd(rolling_shutter_time != 0)*/,
                     const float* sample_times /*[S] device, desc->shared_list only (NULL otherwise)*/,
                     float* out_img /*S*H*W*3*/, float* out_T /*S*H*W*/, float* out_depth,
                     float* out_combined /*NULL, or H*W*3: gs_combine_fwd(desc->combine_gamma, desc->combine_min_level) of
                     out_img, launched by this call (see gs_frame_desc)*/,
                     void* arena, long long arena_bytes, void* host_pinned,
                     long long host_pinned_bytes, gs_frame_state* state, void* stream);
long long gs_frame_backward_bytes(const gs_frame_state* state);
/* v_records [P*N*12] (rows the compositor never touched are left as they are), touched [P*N] u8 zeroed by the caller;
 * v_img / cmb_* / bwd_variant as in gs_rasterize_bwd_slice; allocates behind state->arena_used of the SAME arena */
int gs_frame_backward(const gs_frame_state* state, const float* records, const float* background, const int* band_edges,
                      const float* out_T, const float* v_img, const float* v_alpha, const float* cmb_scale,
                      float cmb_gamma, float cmb_min_level, int bwd_variant, float* v_records, unsigned char* touched,
                      const float* pix_vel /*as in the forward*/, const float* sample_times /*as in the forward*/,
                      void* arena, long long arena_bytes, void* stream);
/* gs_frame_backward with a depth gradient: v_depth [S*H*W] or NULL = d loss / d out_depth of the forward (per sample image
 * the sum over the blended splats of weight * camera-space depth; depth is a fourth colour channel with background 0).
 * Non-NULL: v_records[.., 11] receives d loss / d record depth (float 9) besides the colour gradients — hand it to the
 * projection backward with grad flag 64.  NULL: exactly gs_frame_backward (which calls this with NULL).  With v_depth,
 * bwd_variant bit 1024 (the splat-parallel measurement form, no depth channel) is not honoured: the depth kernel runs
 * (the dispatch rule of csrc/raster_bwd.hip). */
int gs_frame_backward_depth(const gs_frame_state* state, const float* records, const float* background,
                            const int* band_edges, const float* out_T, const float* v_img, const float* v_alpha,
                            const float* cmb_scale, float cmb_gamma, float cmb_min_level, int bwd_variant,
                            float* v_records, unsigned char* touched, const float* pix_vel, const float* sample_times,
                            void* arena, long long arena_bytes, const float* v_depth /*[S*H*W] or NULL*/, void* stream);
/* Absgrad output of a frame backward run with bwd_variant + GS_BWD_ABSGRAD: out[b][i] = the sum over camera b's
 * sub-poses [b*P/cameras, (b+1)*P/cameras), in sub-pose order, of v_records[p*N+i][9..10], rows with touched[p*N+i] only.
 * Every row of out [cameras,N,2] is stored, zeros included (out may arrive uninitialised).  One ordered launch, no
 * atomics.  Densification statistic of AbsGS / gsplat's `absgrad`; same unit as v_xy_sum (pixels). */
int gs_xy_absgrad_sum(int N, int P, int cameras, const float* v_records /*[P*N,12]*/,
                      const unsigned char* touched /*[P*N]*/, float* out /*[cameras*N*2]*/, void* stream);
/* measurement only (not thread-safe): HIP events around the stages of the two calls above.  stage_mask bit i enables
 * stage i of {depth_sort, count_scan, slice_plan, slice_count, emit, tile_sort, bin_edges, raster_fwd, slice_sat,
 * raster_bwd, grad_reduce}; gs_frame_profile_read drains the pairs recorded since the last call (synchronising on
 * them) into stage_ids / ms and returns how many it wrote. */
int gs_frame_profile_enable(unsigned stage_mask);
int gs_frame_profile_read(int max_events, int* stage_ids, float* ms);

/* ---- the step after the path: image loss + optimizer ---------------------------------------------
 * Replaces what the nerfstudio fork's trainer runs right after get_outputs (reached from /root/reference/train.py:115-122):
 * splatfacto's loss  L = (1 - lambda) * mean|gt - pred| + lambda * (1 - SSIM(pred, gt))  (pytorch_msssim SSIM: 11x11
 * Gaussian window, sigma 1.5, valid convolution, C1 = 0.01^2, C2 = 0.03^2, mean over the map) together with its
 * backward, and torch.optim.Adam(eps = 1e-15) over the parameter groups. */
long long gs_image_loss_workspace_bytes(int img_height, int img_width);
/* pred, gt, v_pred [H,W,3] fp32 (device); v_pred = d loss / d pred; loss_out[3] = {loss, mean |gt - pred|, mean SSIM}
 * (device).  ssim_lambda == 0: L1 only (any size); otherwise both sides must be >= 11. */
int gs_image_loss_fwd_bwd(int img_height, int img_width, const float* pred, const float* gt, float ssim_lambda,
                          float* v_pred, float* loss_out, void* workspace, long long workspace_bytes, void* stream);
/* ONE Adam step over count (<= 8) tensors; params / grads / exp_avg / exp_avg_sq: HOST arrays of device pointers,
 * numel / lr: host arrays; step = 1-based count of this update (bias corrections 1 - beta^step):
 *   m = m + (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps) */
int gs_adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const long long* numel, const float* lr, double beta1, double beta2, double eps,
                 int step, void* stream);
/* Adam on the rows r of N with mask[r] != 0 only ("selective" Adam: gsplat's SelectiveAdam, Taming-3DGS's sparse
 * optimizer); tensors share N rows, tensor t has widths[t] >= 0 floats per row (0: the tensor is
 * skipped and its pointers may be null, as gs_adam_step skips numel 0; no upper limit); count <= 8; params / grads /
 * exp_avg / exp_avg_sq / widths / lr: HOST arrays (device pointers in the first four).
 * Masked-off rows: parameter, exp_avg and exp_avg_sq are not written (bit-unchanged), the gradient is ignored.
 * Selected elements get exactly gs_adam_step's arithmetic and roundings (same step / bias-correction scalars):
 * bit-identical to what gs_adam_step writes for the same inputs.
 * The selected rows are compacted on the device (prefix sum), so the work scales with their number and nothing is
 * read back; ws: gs_adam_step_rows_workspace_bytes(N) bytes of device scratch.  N == 0 is a no-op. */
int gs_adam_step_rows(int count, int N, const unsigned char* mask /*N*/, float* const* params,
                      const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const int* widths, const float* lr, double beta1, double beta2, double eps, int step,
                      void* ws, long long ws_bytes, void* stream);
long long gs_adam_step_rows_workspace_bytes(int N);
/* mask[r] = 1 if radii[p*N + r] > 0 for any of the M planes, else 0 (gsplat's visibility rule); radii int32 [M*N]. */
int gs_visible_rows(int M, int N, const int* radii, unsigned char* mask, void* stream);

/* ---- 3DGS-MCMC densification (Kheradmand et al. 2024; gsplat's MCMCStrategy, formulas recollected from gsplat 1.x
 * relocation.cu / strategy/ops.py): mcmc.py drives them.  No allocation, no state; both return 0 on success.
 *
 * means[r] += Sigma_r * (z_r * gate_r * scaler) for r < N, in place, one launch: Sigma = R(q/|q|) diag(exp(ls))^2 R^T
 * from the RAW parameters (log-scales [N,3], unnormalised wxyz quaternions [N,4], 16-byte aligned), gate =
 * 1 / (1 + exp(100 (sigmoid(logit) - 0.005))).  z_r: three standard normals, Box-Muller over the four words of
 * Philox4x32-10 with counter (r, 0, step_lo, step_hi) and key (seed_lo, seed_hi) — a function of (seed, step, r) alone —
 * or, when noise_in [N,3] is given, the caller's.  noise_out [N,3] (optional) receives the normals used.  N == 0 is a
 * no-op. */
int gs_mcmc_inject_noise(int N, float* means, const float* log_scales, const float* quats, const float* opacity_logits,
                         float scaler, long long seed, long long step, const float* noise_in, float* noise_out,
                         void* stream);
/* per sampled row i < M: new_opacities[i] = 1 - (1 - o)^(1/n), new_scales[i] = scales[i] * o / D with
 * D = sum_{k<n} C(n,k+1) (-1)^k o'^(k+1) / sqrt(k+1), n = ratios[i] clamped to [1, 51]; opacities [M] and scales [M,3]
 * in LINEAR units, ratios int32 [M]; D is summed in double.  M == 0 is a no-op. */
int gs_mcmc_relocation(int M, const float* opacities, const float* scales, const int* ratios, float* new_opacities,
                       float* new_scales, void* stream);

/* ---- bilateral-grid colour correction (Chen et al. 2007; per-image learned grids as in gsplat's lib_bilagrid / nerfstudio
 * splatfacto's use_bilateral_grid, formulas recollected; csrc/bilagrid_math.h): bilagrid.py drives them.  No allocation,
 * no state, no float atomics: every sum has a fixed order, two runs agree bit for bit.
 *
 * grids [G,12,L,GH,GW] fp32, the 12 channels a row-major 3x4 affine [A | b]; GW, GH, L >= 2.  grid_idx int32 [B] (device)
 * names each image's grid; two images may share one; an index outside [0, G) passes its image through unchanged (out =
 * rgb, v_rgb = v_out, no grid gradient).  Pixel (x, y) of image b samples its grid at ((x + 0.5) / W, (y + 0.5) / H,
 * 0.299 r + 0.587 g + 0.114 b of rgb), each clamped to [0, 1], trilinear with align_corners semantics, and out = A rgb + b.
 * rgb, out, v_out, v_rgb [B,H,W,3].  Any H, W >= 1.  B == 0 or G == 0 is a no-op.  Returns 1 when no tile of the frame
 * fits its lattice footprint in LDS (L beyond about 190). */
int gs_bilagrid_slice_fwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids, const int* grid_idx,
                          const float* rgb, float* out, void* stream);
/* scratch of gs_bilagrid_slice_bwd: one partial row per workgroup (7 MB at 1080p with the 16x16x8 grid); -1 on invalid
 * arguments */
long long gs_bilagrid_slice_bwd_workspace_bytes(int B, int H, int W, int G, int GW, int GH, int L);
/* v_rgb = d loss / d rgb (through A and through the guide, the latter zero where the guide left (0, 1)); v_grids
 * [G,12,L,GH,GW] = d loss / d grids: EVERY value is stored, zeros included for grids no image selected (v_grids may arrive
 * uninitialised).  ws: 16-byte aligned, gs_bilagrid_slice_bwd_workspace_bytes of the same arguments. */
int gs_bilagrid_slice_bwd(int B, int H, int W, int G, int GW, int GH, int L, const float* grids, const int* grid_idx,
                          const float* rgb, const float* v_out, float* v_rgb, float* v_grids, void* ws,
                          long long ws_bytes, void* stream);
/* loss_out[0] (device) = weight * tv(grids), tv = 2 (m_x + m_y + m_z) with m_a the mean over images, channels and
 * positions of the squared forward difference along lattice axis a; v_grids += weight * d tv / d grids (NULL: value
 * only).  The value is summed in double.  ws: 8-byte aligned.  G == 0 is a no-op. */
long long gs_bilagrid_tv_workspace_bytes(int G, int GW, int GH, int L);
int gs_bilagrid_tv_fwd_bwd(int G, int GW, int GH, int L, const float* grids, float weight, float* loss_out,
                           float* v_grids, void* ws, long long ws_bytes, void* stream);

/* ---- colour-corrected evaluation metrics (mip-NeRF 360's color_correct as in gsplat's lib_bilagrid / nerfstudio
 * splatfacto's color_corrected_metrics, recollected; csrc/colorcorrect_math.h states the algorithm): colorcorrect.py drives
 * it.  No allocation, no state, no float atomics: every sum is float64 in an order fixed by (H, W), so two runs agree bit
 * for bit and an image's result does not depend on the rest of the batch.
 *
 * img, ref, out [B,H,W,3] fp32 (out neither img nor ref).  Each of the B pairs is fitted on its own: num_iters times, per
 * output channel c the quadratic warp w_c of the features (rr, rg, rb, gg, gb, bb, r, g, b, 1) that minimises the squared
 * error to ref[c] over the pixels whose img[c], current x[c] and ref[c] all lie in [float(eps), float(1 - eps)]; then x <-
 * clip(a . w, 0, 1) for every pixel, stored as fp32.  A channel with fewer than 10 such pixels or a numerically
 * rank-deficient normal matrix keeps the identity warp for that iteration.  out = x after the last iteration (num_iters
 * == 0: a copy of img).  warps (NULL: not wanted) double [B,num_iters,3,10] receives every fitted warp.  ws: 8-byte
 * aligned, gs_color_correct_workspace_bytes(B, H, W) bytes (-1 on invalid arguments; 1.6 MB per 1080p image).  All
 * iterations run in this one call, nothing is read back.  B == 0 is a no-op; H * W <= 2^30, B <= 65535. */
long long gs_color_correct_workspace_bytes(int B, int H, int W);
int gs_color_correct(int B, int H, int W, const float* img, const float* ref, int num_iters, double eps, float* out,
                     double* warps, void* ws, long long ws_bytes, void* stream);

/* ---- exact k nearest neighbours of a point cloud against itself (csrc/knn_math.h states the algorithm and why it is
 * exact; knn.py drives it): the scale of a Gaussian started from a seed cloud is the mean distance to its 3 nearest
 * neighbours.  No allocation, no state, no float atomics; memory is linear in N.
 *
 * xyz [N,3] fp32, finite.  For every row i: the k smallest (squared distance, index) pairs over the rows j != i, a row
 * excluded by index (a duplicate point is a neighbour at distance 0); d2 = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j in
 * fp32 without fused multiply-add.  dists [N,k] receives the square roots, ascending; idx [N,k] (NULL: not wanted) the
 * rows.  The values do not depend on the order of the rows or on scheduling.  1 <= k <= 16, k < N <= 2^26.
 * cell_size <= 0: chosen on the device (twice the median k-th neighbour distance of <= 1024 fixed-stride rows); either
 * way at least extent / 2^21.  max_rings <= 0: 8.  Rows still open after max_rings shells of the hashed grid are resolved
 * by brute force.  stats (device, NULL: not wanted) receives 4 ints: the cell size (fp32 bits), max_rings, the number of
 * brute-force rows, log2 of the bucket count.  ws: 256-byte aligned, gs_knn_workspace_bytes(N, k) bytes (-1 on invalid
 * arguments; 60 to 80 bytes per row).  Everything runs in this one call, nothing is read back. */
long long gs_knn_workspace_bytes(int N, int k);
int gs_knn(int N, const float* xyz, int k, float cell_size, int max_rings, float* dists, int* idx, int* stats, void* ws,
           long long ws_bytes, void* stream);

/* ---- per-frame blur statistics of a point cloud under the motion model (csrc/blur_math.h states every formula;
 * blurscore.py drives it): how many pixels the camera's twist smears a frame by during its exposure, and how far its
 * rolling shutter shears it.  No allocation, no state, no atomics; two runs agree bit for bit.
 *
 * points [N,3] fp32; per frame f: viewmats [F,16] row-major world-to-camera (OpenCV axes), lin / ang [F,3] the camera's
 * body twist in that frame, intrins [F,4] = fx fy cx cy, times [F,2] = exposure E, readout T.  For every pair, in fp32
 * without fused multiply-add: pc = V p, (u, v) its pixel, pv its pixel velocity (the renderer's pixel_velocity),
 * blur = E |pv|, skew = T |pv| |v / H - 1/2|.  A pair is visible iff pc.z > clip and 0 <= u < W and 0 <= v < H.  Over
 * the visible pairs of frame f: counts[f] their number, stats[f*4 ..] = mean blur, rms blur, max blur, mean skew (sums in
 * float64, in an order fixed by N); all zero when no pair is visible.  F == 0 or N == 0 launch nothing (N == 0 clears
 * counts and stats).  F <= 65535 * 32, N <= 2^30, W, H >= 1; anything else is GS_ERR_INVALID before any launch.
 * ws: 8-byte aligned, gs_blur_stats_workspace_bytes(F, N) bytes (-1 on invalid arguments; 32 bytes per frame and 1024
 * points).  gs_blur_stats_ppt is the same call with the points a thread keeps in registers chosen by the caller (1, 2, 4,
 * 8, 16; <= 0: the default) — a tuning knob that reorders the float64 sums and nothing else. */
long long gs_blur_stats_workspace_bytes(int F, int N);
int gs_blur_stats(int F, int N, const float* points, const float* viewmats, const float* lin, const float* ang,
                  const float* intrins, const float* times, int W, int H, float clip, int* counts, float* stats,
                  void* ws, long long ws_bytes, void* stream);
int gs_blur_stats_ppt(int F, int N, const float* points, const float* viewmats, const float* lin, const float* ang,
                      const float* intrins, const float* times, int W, int H, float clip, int points_per_thread,
                      int* counts, float* stats, void* ws, long long ws_bytes, void* stream);

/* ---- scale- and shift-invariant depth-prior loss (csrc/depthprior_math.h states every formula; depthprior.py drives
 * it): a monocular depth prior, known up to scale and shift, against the rendered depth.  No allocation, no state, no
 * atomics, two launches, nothing read back; two runs agree bit for bit and a frame's results do not depend on the rest
 * of the batch.
 *
 * depth_acc, alphas [B,S,H,W] fp32: the compositor's per-sample sums (weight * camera-space depth; 1 - transmittance).
 * prior [B,H,W] fp32, 0 (or less): no value.  Per pixel, in fp32 without fused multiply-add: d = the samples of depth_acc
 * added in order, divided by S; a likewise; valid iff prior > 0 and a > min_alpha (and d > 0 with space 1); x = d / a
 * (space 0, depth) or a / d (space 1, disparity); y = prior.  Over the valid pixels of frame b, in float64 in an order
 * fixed by H * W: n, sum x, sum y, sum xx, sum yy, sum xy (and sum |x - y| for kind 1).
 * kind 0 (pearson): loss_out[b] = weight * (1 - rho), rho = (n sxy - sx sy) / sqrt((n sxx - sx^2)(n syy - sy^2)); with
 * n < 2, or either variance term not above 1e-12 * n * sxx (syy), the loss and every gradient are exactly 0.
 * kind 1 (l1): loss_out[b] = weight * sum |x - y| / max(n, 1).
 * v_depth_acc, v_alphas [B,S,H,W] receive d loss_out[b] / d depth_acc, d alphas (float64 chain, rounded once; the same
 * value for every sample of a pixel; exact zeros at invalid pixels).  stats_out [B*8] float64: the seven sums, then rho
 * (0 for kind 1 or a degenerate frame).  1 <= S, B * S <= 256, H, W >= 1, B * S * H * W < 2^30, min_alpha >= 0, kind and
 * space 0 or 1; anything else is GS_ERR_INVALID before any launch.  B == 0 launches nothing.  ws: 8-byte aligned,
 * gs_depth_prior_workspace_bytes(B, S, H, W) bytes (-1 on invalid arguments; 56 bytes per frame and 4096 pixels). */
long long gs_depth_prior_workspace_bytes(int B, int S, int H, int W);
int gs_depth_prior_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* prior,
                        int kind, int space, float min_alpha, float weight, float* loss_out, double* stats_out,
                        float* v_depth_acc, float* v_alphas, void* ws, long long ws_bytes, void* stream);

/* ---- TSDF fusion of depth maps and marching-tetrahedra mesh extraction (csrc/tsdf_math.h states the update rule, the
 * tetrahedra and every order; tsdf.py drives it).  No allocation, no state, no atomics, no workgroup waits on another;
 * two runs agree bit for bit.
 *
 * The volume: tsdf, weight [nz,ny,nx] fp32, color [nz,ny,nx,3] fp32 or NULL, x fastest; sample (i, j, k) sits at
 * (ox, oy, oz) + voxel_size * (i, j, k).  2 <= nx, ny, nz <= 1024 and nx * ny * nz <= 2^30.
 *
 * gs_tsdf_integrate updates the volume in place from B frames: depth [B,H,W] camera-space z, viewmats [B,16] row-major
 * world-to-camera (OpenCV axes, +z forward), intrins [B,4] = fx fy cx cy, color_images [B,H,W,3] (given exactly when
 * color is), weight_images [B,H,W] or NULL (1).  Per voxel, frames in index order, fp32 without fused multiply-add:
 * p = R x + t, skip if p.z <= 0; u = fx p.x / p.z + cx, v likewise, the pixel is (floor u, floor v), skip outside the
 * image; D, w the pixel's depth and weight, skip unless D is finite, depth_min < D <= depth_max and w > 0;
 * sdf = D - p.z, skip if sdf < -trunc; val = min(1, sdf / trunc); Wn = W + w; tsdf = (tsdf W + val w) / Wn, colour
 * likewise; W = min(Wn, max_weight).  A voxel no frame touched is not written.  One launch per 16 frames; the result does
 * not depend on how B is cut into calls.  B == 0 launches nothing.  H, W <= 16384, trunc > 0, max_weight > 0,
 * voxel_size > 0; anything else, or a null pointer, is GS_ERR_INVALID before any launch.
 *
 * Extraction is two calls because V and F size the outputs.  gs_tsdf_mesh_count leaves V and F in counts (device, 2
 * ints; -1: more than an int holds) and what gs_tsdf_mesh_emit needs in ws; the caller reads counts back, allocates
 * verts [V,3] fp32, faces [F,3] int32 and colors [V,3] fp32 (NULL: not wanted; needs color) and calls
 * gs_tsdf_mesh_emit with the same volume, level and ws.  A corner is inside when tsdf < level; a cell is used
 * when its 8 corners have weight > min_weight.  Vertices are ordered by (owner sample, edge type), faces by (cell,
 * tetrahedron, triangle); every vertex is referenced.  V == 0 and F == 0 launch nothing in emit.  ws: 256-byte aligned,
 * gs_tsdf_mesh_workspace_bytes(nx, ny, nz) bytes (-1 on invalid arguments; a little over 6 bytes per sample). */
int gs_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float* tsdf, float* weight,
                      float* color, int B, int H, int W, const float* depth, const float* viewmats, const float* intrins,
                      const float* color_images, const float* weight_images, float trunc, float depth_min,
                      float depth_max, float max_weight, void* stream);
long long gs_tsdf_mesh_workspace_bytes(int nx, int ny, int nz);
int gs_tsdf_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float level, float min_weight,
                       int* counts, void* ws, long long ws_bytes, void* stream);
int gs_tsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf,
                      const float* color, float level, int V, int F, float* verts, int* faces, float* colors, void* ws,
                      long long ws_bytes, void* stream);

/* ---- normals from the rendered depth, normal-prior and normal smoothness loss (csrc/normal_math.h states every formula;
 * normals.py drives it).  No allocation, no state, no atomics, nothing read back; two runs agree bit for bit and a
 * frame's results do not depend on the rest of the batch.
 *
 * depth_acc, alphas [B,S,H,W] fp32: the compositor's per-sample sums, d and a their sample means as in
 * gs_depth_prior_loss.  intrins [B,4] fp32 (device) = fx fy cx cy of the camera each frame was rendered with.  Per pixel
 * (u, v), in fp32 without fused multiply-add: has_z iff a > min_alpha and d > 0, z = d / a, P = (rx z, ry z, z) with
 * rx = ((u + 0.5) - cx) / fx, ry = ((v + 0.5) - cy) / fy.  A pixel with 1 <= u <= W - 2, 1 <= v <= H - 2 whose own has_z
 * and that of its four axis neighbours hold has tx = P(u+1,v) - P(u-1,v), ty = P(u,v+1) - P(u,v-1), c = ty x tx,
 * l2 = c.c, and, iff l2 > 1e-30f, the normal n = c / sqrt(l2): camera frame (x right, y down, z forward), facing the
 * camera.  normals_out [B,H,W,3] fp32 receives it, (0,0,0) where there is none.
 *
 * gs_depth_normals: that, in one launch.
 *
 * gs_normal_loss: two launches.  prior [B,H,W,3] fp32 or NULL: a pixel whose vector has a squared length that is 0 or not
 * finite in fp32 has no value; the others are normalised, m.  guide [B,H,W,3] fp32 or NULL (ignored with edge_beta == 0).
 * Over frame b in float64, in an order fixed by H and W: Np pixels with a normal and a prior value and their sum of
 * 1 - n.m; Ns horizontally or vertically adjacent pairs (p, q) of normals, their sum of g (1 - n_p.n_q) and of g, with
 * g = exp(-edge_beta (|dI_r| + |dI_g| + |dI_b|) / 3) of the guide in fp32, or 1.
 * loss_out[b] = prior_weight sum(1 - n.m) / max(Np, 1) + smooth_weight sum g (1 - n_p.n_q) / max(Ns, 1).
 * stats_out [B*6] float64: the number of normals, Np, sum(1 - n.m), Ns, sum g (1 - n_p.n_q), sum g.
 * v_depth_acc, v_alphas [B,S,H,W] receive d loss_out[b] / d depth_acc, d alphas (float64 chain, rounded once; the same
 * value for every sample of a pixel; exact zeros at pixels without has_z and for a term whose count is 0).
 * normals_out may be NULL.  1 <= S, B * S <= 256, H, W >= 1, B * S * H * W < 2^30, min_alpha >= 0, edge_beta >= 0;
 * anything else, or a null pointer where none is allowed, is GS_ERR_INVALID before any launch.  B == 0 launches nothing.
 * ws: 8-byte aligned, gs_normal_loss_workspace_bytes(B, S, H, W) bytes (-1 on invalid arguments; 20 bytes per pixel and
 * 48 bytes per frame and 256 x 8 pixels). */
int gs_depth_normals(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* intrins,
                     float min_alpha, float* normals_out, void* stream);
long long gs_normal_loss_workspace_bytes(int B, int S, int H, int W);
int gs_normal_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* intrins,
                   const float* prior, const float* guide, float prior_weight, float smooth_weight, float edge_beta,
                   float min_alpha, float* loss_out, double* stats_out, float* normals_out, float* v_depth_acc,
                   float* v_alphas, void* ws, long long ws_bytes, void* stream);

/* ---- mesh clean-up: connected components of a triangle mesh and the removal of small ones (csrc/meshclean_math.h states
 * the graph, the rounds, the ranking and the survivor rule; meshclean.py drives it).  No allocation, no state; integer
 * atomics only (atomicMin, atomicAdd), no workgroup waits on another; two runs agree bit for bit.
 *
 * faces [F,3] int32, labels [V] int32, counts 8 ints, all on the device.  1 <= V, 0 <= F.  Every kernel tests the three
 * indices of a face against [0, V) before it uses them; a face that fails is left out and counts[4] (status) becomes 1.
 * A label outside [0, V) met by finish makes it 2.  counts: [0] V', [1] F', [2] C, [3] kept, [4] status, [5] the number
 * (round + 1) of the last round that hooked.
 *
 * gs_mesh_components_round(round): round 0 first sets labels[v] = v and counts = 0; then one hook launch over the faces
 * and one compress launch over the vertices.  The caller reads counts[5] back after every round and stops when it is not
 * round + 1; labels[v] is then the smallest vertex index of v's component.  round >= 8 * bit_length(V) + 8 is refused.
 * gs_mesh_components_finish: faces and vertices per component and the table of the C components in ascending order of
 * their label, left in ws; counts[2] = C.  gs_mesh_components_table copies the first C rows of that table out.
 * gs_mesh_filter_plan (after finish, same ws): the components with at least one face are ranked by (face count
 * descending, label ascending); keep_largest = K > 0 lets only the first min(K, C) through (0: all), of these the ones
 * with fewer than min_faces faces are dropped; output positions of the surviving vertices and faces are left in ws,
 * counts[0] = V', counts[1] = F', counts[3] = surviving components.  The caller reads counts back once, allocates
 * verts_out [V',3] fp32, faces_out [F',3] int32, colors_out [V',3] fp32 (given exactly when colors is) and calls
 * gs_mesh_filter_emit (same ws): surviving vertices and faces in their old relative order, faces re-indexed.  V' == 0 and
 * F' == 0 launch nothing.  plan and emit need F >= 1.
 * Anything else, or a null pointer where none is allowed, is GS_ERR_INVALID before any launch.  ws: 256-byte aligned,
 * gs_mesh_clean_workspace_bytes(V, F) bytes (-1 on invalid arguments; 32 bytes per vertex and 4 per face). */
long long gs_mesh_clean_workspace_bytes(int V, int F);
int gs_mesh_components_round(int V, int F, const int* faces, int* labels, int round, int* counts, void* stream);
int gs_mesh_components_finish(int V, int F, const int* faces, const int* labels, int* counts, void* ws, long long ws_bytes,
                              void* stream);
int gs_mesh_components_table(int V, int F, int C, int* roots, int* face_counts, int* vert_counts, const void* ws,
                             long long ws_bytes, void* stream);
int gs_mesh_filter_plan(int V, int F, const int* faces, const int* labels, int min_faces, int keep_largest, int* counts,
                        void* ws, long long ws_bytes, void* stream);
int gs_mesh_filter_emit(int V, int F, const float* verts, const int* faces, const float* colors, const int* labels,
                        int V_out, int F_out, float* verts_out, int* faces_out, float* colors_out, const void* ws,
                        long long ws_bytes, void* stream);

/* ---- mesh decimation: vertex clustering on a grid of cell_size anchored at the world origin, one representative per
 * cluster placed by its plane quadrics (csrc/meshdecimate_math.h states the cell, the cluster order, the representative
 * and the face rule; meshdecimate.py drives it).  No allocation, no state, no float atomics, no workgroup waits on
 * another; every word of ws is written before it is read: two runs agree bit for bit whatever ws held.
 *
 * The arguments travel in a descriptor, the stream as its last field.  1 <= V <= 2^30, 1 <= F <= (2^31 - 1) / 3; verts [V,3] fp32, faces [F,3]
 * int32, colors [V,3] fp32 or NULL, cell_size > 0 and finite, counts 8 ints, all pointers on the device.  ws: 256-byte
 * aligned, gs_mesh_decimate_workspace_bytes(V, F) bytes (a pure host call; -1 on sizes outside the limits).
 * gs_mesh_decimate_plan does everything that decides the output sizes and leaves in counts: [0] V', [1] F', [2] the
 * clusters, [3] the faces dropped as degenerate, [4] the faces dropped as duplicates (dedupe != 0), [5] status: 0, 1 (a
 * face index outside [0, V); tested before it is used) or 2 (a coordinate that is not finite, or a cell index beyond
 * +-2^30).  With a status the other words mean nothing.  plan reads neither the outputs nor V_out / F_out.
 * gs_mesh_decimate_emit (same descriptor, same ws, V_out = V', F_out = F' as read back) writes verts_out [V',3] fp32,
 * colors_out [V',3] fp32 (NULL, or given with colors), faces_out [F',3] int32 and cluster_of [V] int32 (NULL, or the
 * output vertex of every input vertex, -1 where its cluster was dropped).  verts_out may be NULL when V' == 0, faces_out
 * when F' == 0.  Anything else is GS_ERR_INVALID before any launch, a short ws GS_ERR_WORKSPACE. */
typedef struct gs_mesh_decimate_desc {
  int V, F;
  const float* verts;
  const int* faces;
  const float* colors;
  double cell_size;
  int dedupe;
  int* counts;
  void* ws;
  long long ws_bytes;
  float* verts_out;
  int* faces_out;
  float* colors_out;
  int* cluster_of;
  int V_out, F_out;
  void* stream;
} gs_mesh_decimate_desc;
long long gs_mesh_decimate_workspace_bytes(int V, int F);
int gs_mesh_decimate_plan(const gs_mesh_decimate_desc* d);
int gs_mesh_decimate_emit(const gs_mesh_decimate_desc* d);

#ifdef __cplusplus
}
#endif
#endif /* GSDEBLUR_H */
