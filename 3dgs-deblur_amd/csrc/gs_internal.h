// gs_internal.h — host-side declarations shared by every translation unit of the library: status codes, the export
// attribute, the variant bits of the compositor entry points and the prototypes of the library-internal (hidden) entry
// points that csrc/frame.hip calls.  The files that DEFINE those entry points include this header too, so a definition
// that drifts from its prototype is a compile error (conflicting types for an extern "C" function).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gsdeblur.h"     // GS_BWD_ABSGRAD, and the exported prototypes (checked against the definitions)

#define GS_OK 0
#define GS_ERR_INVALID 1
#define GS_ERR_WORKSPACE 3
// launch errors are returned as 1000 + hipError_t

#define GS_EXPORT extern "C" __attribute__((visibility("default")))

static inline int gs_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GS_OK : 1000 + (int)e;
}

// `variant` of the compositor entry points (gs_rasterize_fwd*, gs_rasterize_bwd*, gs_frame_desc.fwd_variant /
// bwd_variant); GS_BWD_ABSGRAD (2048) is public: include/gsdeblur.h
constexpr int GS_VARIANT_ROUND1_PLAIN = 1;   // forward: the round-1 kernel without the empty-tile skip (test library only)
constexpr int GS_VARIANT_ROUND1 = 2;         // the round-1 kernels (test library only)
constexpr int GS_VARIANT_CLAMP_GRAD = 256;   // backward: the upstream alpha-clamp gradient (stripped before dispatch)
constexpr int GS_VARIANT_SPLAT = 1024;       // backward: the splat-parallel measurement form

// Library-internal forms of three exported entry points, with a depth gradient (and, for the SE(3) compositor, a camera
// count).  Defined in raster_bwd.hip / raster_rs.hip next to the exported forms, which forward to them.
extern "C" int gs_rasterize_bwd_slice_depth(const float* records, const int* sorted_vals, const int* tile_bins,
                                            const int* band_edges, const float* background, int S, int R, int H, int W,
                                            const float* out_T, const int* final_idx, const float* v_img,
                                            const float* v_alpha, float* bwd_T, float* bwd_B, float* v_records,
                                            const int* gi_of_e, float* tuples, unsigned char* flags,
                                            const int* sorted_ids, int n_records, const unsigned char* tile_hot,
                                            int variant, const float* cmb_scale, float cmb_gamma, float cmb_min_level,
                                            const float* v_depth, int cameras, void* stream);
extern "C" int gs_rasterize_bwd_rs_slice_depth(const float* records, const int* sorted_vals, const int* tile_bins,
                                               const int* band_edges, const float* background, int S, int H, int W,
                                               const float* out_T, const int* final_idx, const float* v_img,
                                               const float* v_alpha, float* bwd_T, float* bwd_B, float* tuples,
                                               unsigned char* flags, const int* sorted_ids, int n_records, int variant,
                                               const float* cmb_scale, float cmb_gamma, float cmb_min_level,
                                               const float* pix_vel, int N, float rolling_shutter_time,
                                               const float* shared_list_times, const float* v_depth, void* stream);
extern "C" int gs_reduce_grad_tuples_depth(int n_slice, const unsigned* slice_gi, const unsigned* counts,
                                           const unsigned* cum_excl, const float* tuples, const unsigned char* flags,
                                           float* v_records, unsigned char* touched, long long n_isect,
                                           const float* records, int tuples_per_entry, int depth, void* stream);
