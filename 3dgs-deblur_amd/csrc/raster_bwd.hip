// raster_bwd.hip — reverse-order backward of the compositor and the atomic-free gradient reduce.
// Split from raster.hip because this translation unit is compiled with -fno-slp-vectorize: left to itself the
// SLP vectoriser packs the four per-pixel chains into v_pk_*_f32 pairs but needs v_mov shuffles to assemble
// them (128 -> 99 VGPRs, -14 % kernel time with SLP off).  The packing that pays is done BY HAND instead
// (hand-packed: the lane's four pixels are two float2 pairs from load to store, non-hit pixels neutralised by
// selects instead of exec regions: ~160 -> ~126 VALU per hit entry, -5 % kernel time measured, run 29).
#include <type_traits>
#include "raster_common.h"

namespace gs {

// ---------------------------------------------------------------------------
// backward compositor (single pass and depth-sliced): reverse-order traversal from each pixel's final
// index, written for a cheap instruction stream:
//   * one predicate per pixel instead of three nested exec-mask regions, exp2 on a pre-scaled
//     exponent, v_rcp_f32 for 1/(1-alpha) (the IEEE division expansion cost ~10 VALU per pixel);
//   * the 9 per-Gaussian wave reductions (54 DPP adds + 18 lane moves) are replaced by a transposed
//     reduction through wave-private LDS: every lane drops its 9 partials into row (g*9+c) of a
//     [36][68] tile (conflict-free ds_write_b32), after 4 Gaussians lanes 0..35 each sum one row
//     with 16 conflict-free ds_read_b128 and park the total in tot[j][c]; at the end of the batch
//     lane j picks up its 9 totals.  ~20 issue slots per Gaussian instead of ~80.
// ---------------------------------------------------------------------------
// The round-1 backward (raster_bwd_kernel_v2 below) is TEST infrastructure since round 4, like the round-1 forward:
// compiled only with -DGS_ROUND1_KERNELS=1 into tests/libgsdeblur_round1.so (see raster.hip).
#ifndef GS_ROUND1_KERNELS
#define GS_ROUND1_KERNELS 0
#endif
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
#if GS_ROUND1_KERNELS
#ifndef GS_RED_G
#define GS_RED_G 3
#endif
constexpr int kRedG = GS_RED_G;             // Gaussians per transposed-reduction group
constexpr int kRedStride = 68;              // floats per row (64 + 4: 16-byte aligned, b128 conflict-free)
constexpr int kRedFloats = kRedG * 9 * kRedStride + 64 * 9;

// OUT = 0: 9 fp32 atomics per (Gaussian, tile) into v_records (gsplat-compatible op: no emission index);
// OUT = 1: no atomics at all — the entry's 9 gradients go to tuples[e] (48 B, e = emission index of the
// entry, so the tuples of one Gaussian are CONTIGUOUS) and flags[e] = 1; gs_reduce_grad_tuples then sums
// each Gaussian's segment.  At ~20 G atomic ops/s the atomics were 40 % of this kernel.
#ifndef GS_BWD_WAVES
#define GS_BWD_WAVES 4   // 128 VGPRs + 38 KB LDS per block -> 4 waves per SIMD (+3.5 % measured)
#endif
template <bool STATE, int OUT>
__global__ __launch_bounds__(256, GS_BWD_WAVES) void raster_bwd_kernel_v2(RasterParams prm, const float* __restrict__ out_T,
                                                            const int* __restrict__ final_idx,
                                                            const float* __restrict__ v_img,
                                                            const float* __restrict__ v_alpha,  // may be null
                                                            float* __restrict__ v_records, unsigned n_blocks,
                                                            float* __restrict__ bwd_T, float* __restrict__ bwd_B,
                                                            float* __restrict__ tuples,
                                                            unsigned char* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) float lds_all[4 * kRedFloats];
  const int lane = lane_id();
  float* red = lds_all + (threadIdx.x >> 6) * kRedFloats;   // wave-private
  float* tot = red + kRedG * 9 * kRedStride;
  const int T = prm.tiles_x * prm.tiles_y;
  const unsigned work = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)(xcd_remap(blockIdx.x, n_blocks) * 4u + (threadIdx.x >> 6)));
  if (work >= (unsigned)(prm.S * T)) return;
  const int s = work / T, t = work % T;
  const int ty = t / prm.tiles_x, tx = t % prm.tiles_x;
  const int p = s * prm.R + find_band(prm.band_edges, prm.R, ty);
  int2 range = prm.tile_bins[(size_t)p * T + t];
  range.x = __builtin_amdgcn_readfirstlane(range.x);
  range.y = __builtin_amdgcn_readfirstlane(range.y);
  if (range.y <= range.x) return;

  const int px = tx * K::kTile + (lane & 15);
  const int py0 = ty * K::kTile + (lane >> 4) * 4;
  const float pxf = (float)px + 0.5f;
  const float bgr = prm.background[0], bgg = prm.background[1], bgb = prm.background[2];

  // per pixel: Tk = transmittance behind the current Gaussian, Dv = (colour accumulated from behind,
  // dotted with v_out) - va, where va = T_final * (v_alpha_out - bg . v_out).  Only the DOT of the
  // behind-colour with v_out is ever needed, so one float replaces the three colour channels.
  float Tk[4], Dv[4], vr[4], vg[4], vb[4], pyf[4];
  int fin[4];
  f2 Tk2[2], Dv2[2], vr2[2], vg2[2], vb2[2], pyf2[2];
  int my_end = range.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = py0 + k;
    pyf[k] = (float)y + 0.5f;
    Tk[k] = 1.f; Dv[k] = 0.f; fin[k] = range.x; vr[k] = vg[k] = vb[k] = 0.f;
    if (px < prm.W && y < prm.H) {
      size_t pix = ((size_t)s * prm.H + y) * prm.W + px;
      const float Tfin = out_T[pix];
      fin[k] = final_idx[pix];
      vr[k] = v_img[pix * 3 + 0]; vg[k] = v_img[pix * 3 + 1]; vb[k] = v_img[pix * 3 + 2];
      if (prm.cmb_scale) {
        // v_img holds the sample image: d loss / d sample = combine_grad(sample, scale) — the arithmetic of
        // combine_bwd_kernel, so the fused and the two-step backward agree bit for bit
        const size_t q = ((size_t)y * prm.W + px) * 3;
        vr[k] = combine_grad(vr[k], prm.cmb_scale[q + 0], prm.cmb_gamma, prm.cmb_min);
        vg[k] = combine_grad(vg[k], prm.cmb_scale[q + 1], prm.cmb_gamma, prm.cmb_min);
        vb[k] = combine_grad(vb[k], prm.cmb_scale[q + 2], prm.cmb_gamma, prm.cmb_min);
      }
      const float va_out = v_alpha ? v_alpha[pix] : 0.f;
      const float va = Tfin * (va_out - (bgr * vr[k] + bgg * vg[k] + bgb * vb[k]));
      Tk[k] = Tfin;
      Dv[k] = -va;
      if (STATE) {
        Tk[k] = bwd_T[pix];
        Dv[k] = bwd_B[pix] - va;
      }
    }
    my_end = max(my_end, fin[k]);
  }
  const int wave_end = __builtin_amdgcn_readfirstlane(wave_max_i(my_end));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    Tk2[h] = f2{Tk[2 * h], Tk[2 * h + 1]}; Dv2[h] = f2{Dv[2 * h], Dv[2 * h + 1]};
    vr2[h] = f2{vr[2 * h], vr[2 * h + 1]}; vg2[h] = f2{vg[2 * h], vg[2 * h + 1]}; vb2[h] = f2{vb[2 * h], vb[2 * h + 1]};
    pyf2[h] = f2{pyf[2 * h], pyf[2 * h + 1]};
  }
  const int* __restrict__ vals = prm.sorted_vals;
  const float kL2E = -1.4426950408889634f;
  const float agm = prm.alpha_grad_max;
  const int row = lane;                        // row-sum role: lanes 0..35
  const int row_g = row / 9, row_c = row - row_g * 9;

  for (int batch_end = wave_end; batch_end > range.x; batch_end -= 64) {
    const int idx = batch_end - 1 - lane;
    const bool valid = idx >= range.x;
    const int eid = valid ? vals[idx] : 0;
    const int gid = (valid && prm.gi_of_e) ? prm.gi_of_e[eid] : eid;
    const Rec9 rec = load_rec(prm.records, gid, valid);
    const float sx = rec.cx * (0.5f * kL2E), sy = rec.cy * kL2E, sz = rec.cz * (0.5f * kL2E);
#pragma unroll
    for (int c = 0; c < 9; ++c) tot[lane * 9 + c] = 0.f;
    const int n = min(64, batch_end - range.x);
    unsigned filled = 0;                          // which slots of the current group hold data
    int g = 0, gbase = 0;                         // slot inside the group, batch position of its first Gaussian
    for (int j = 0; j < n; ++j, ++g) {
      const int idx_j = batch_end - 1 - j;
      const float gx = readlane_f(rec.x, j), gy = readlane_f(rec.y, j);
      const float qx = readlane_f(sx, j), qy = readlane_f(sy, j), qz = readlane_f(sz, j);
      const float op = readlane_f(rec.op, j);
      const float dx = gx - pxf;
      const float hx = qx * dx * dx;             // exponent terms, pre-scaled by -log2(e)
      const float bx = qy * dx;
      // hand-packed variant: the four pixels of a lane are two float2 pairs, every multiply-add of the hit
      // part is one v_pk_*_f32 per pair; pixels that are not hit are neutralised by SELECTING alpha = 0
      // (1/(1-0) = 1 exactly, every contribution is an exact zero) instead of per-pixel exec regions
      f2 dy2[2], vis2[2], ov2[2];
      bool hit[4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        dy2[h] = gy - pyf2[h];
        const f2 s2 = hx + dy2[h] * (bx + qz * dy2[h]);
        vis2[h] = f2{__builtin_amdgcn_exp2f(s2.x), __builtin_amdgcn_exp2f(s2.y)};
        ov2[h] = op * vis2[h];
        hit[2 * h] = (idx_j < fin[2 * h]) && (s2.x <= 0.f) && (fminf(K::kAlphaMax, ov2[h].x) >= K::kAlphaMin);
        hit[2 * h + 1] = (idx_j < fin[2 * h + 1]) && (s2.y <= 0.f) && (fminf(K::kAlphaMax, ov2[h].y) >= K::kAlphaMin);
      }
      if (__ballot(hit[0] || hit[1] || hit[2] || hit[3]) != 0ull) {
        const float cx = readlane_f(rec.cx, j), cy = readlane_f(rec.cy, j), cz = readlane_f(rec.cz, j);
        const float cr = readlane_f(rec.r, j), cg = readlane_f(rec.g, j), cb = readlane_f(rec.b, j);
        const float hdx2 = 0.5f * dx * dx;
        const float cxdx = cx * dx, cydx = cy * dx;
        f2 q_x = {0.f, 0.f}, q_y = q_x, q_cx = q_x, q_cy = q_x, q_cz = q_x, q_op = q_x, q_r = q_x, q_g = q_x, q_b = q_x;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool h0 = hit[2 * h], h1 = hit[2 * h + 1];
          const f2 alpha = {h0 ? fminf(K::kAlphaMax, ov2[h].x) : 0.f, h1 ? fminf(K::kAlphaMax, ov2[h].y) : 0.f};
          const f2 om = 1.f - alpha;
          const f2 ra = {__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};
          Tk2[h] *= ra;                          // transmittance in front of this Gaussian
          const f2 fac = alpha * Tk2[h];
          q_r += fac * vr2[h]; q_g += fac * vg2[h]; q_b += fac * vb2[h];
          const f2 cv = cr * vr2[h] + cg * vg2[h] + cb * vb2[h];
          const f2 v_al = Tk2[h] * cv - ra * Dv2[h];
          Dv2[h] += fac * cv;
          // d min(0.999, o*vis) = 0 when clamped
          const bool f0 = h0 && ov2[h].x <= agm, f1 = h1 && ov2[h].y <= agm;
          const f2 ovm = {f0 ? ov2[h].x : 0.f, f1 ? ov2[h].y : 0.f};
          const f2 vism = {f0 ? vis2[h].x : 0.f, f1 ? vis2[h].y : 0.f};
          const f2 v_sigma = -ovm * v_al;
          q_op += vism * v_al;
          const f2 vsdy = v_sigma * dy2[h];
          q_cx += v_sigma * hdx2;
          q_cy += vsdy * dx;
          q_cz += vsdy * dy2[h];                 // * 0.5 below
          q_x += v_sigma * (cxdx + cy * dy2[h]);
          q_y += v_sigma * (cydx + cz * dy2[h]);
        }
        const float p_x = q_x.x + q_x.y, p_y = q_y.x + q_y.y, p_cx = q_cx.x + q_cx.y, p_cy = q_cy.x + q_cy.y,
                    p_cz = 0.5f * (q_cz.x + q_cz.y), p_op = q_op.x + q_op.y, p_r = q_r.x + q_r.y,
                    p_g = q_g.x + q_g.y, p_b = q_b.x + q_b.y;
        filled |= 1u << g;
        float* r0 = red + g * (9 * kRedStride) + lane;
        r0[0 * kRedStride] = p_x;  r0[1 * kRedStride] = p_y;  r0[2 * kRedStride] = p_cx;
        r0[3 * kRedStride] = p_cy; r0[4 * kRedStride] = p_cz; r0[5 * kRedStride] = p_op;
        r0[6 * kRedStride] = p_r;  r0[7 * kRedStride] = p_g;  r0[8 * kRedStride] = p_b;
      }
      if (g == kRedG - 1 || j == n - 1) {
        if (filled) {
          __builtin_amdgcn_wave_barrier();
          if (row < kRedG * 9 && ((filled >> row_g) & 1u)) {
            const f4* rp = reinterpret_cast<const f4*>(red + row * kRedStride);
            f4 a0 = rp[0], a1 = rp[1], a2 = rp[2], a3 = rp[3];
#pragma unroll
            for (int q = 4; q < 16; q += 4) { a0 += rp[q]; a1 += rp[q + 1]; a2 += rp[q + 2]; a3 += rp[q + 3]; }
            const f4 v = (a0 + a1) + (a2 + a3);
            const float sum = (v.x + v.y) + (v.z + v.w);
            const int jj = gbase + row_g;                   // batch position of this row's Gaussian
            tot[jj * 9 + row_c] = sum;
          }
          __builtin_amdgcn_wave_barrier();
          filled = 0;
        }
        g = -1;
        gbase = j + 1;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (valid) {
      float a[9];
      bool nz = false;
#pragma unroll
      for (int c = 0; c < 9; ++c) { a[c] = tot[lane * 9 + c]; nz |= a[c] != 0.f; }
      if (OUT == 1) {
        if (nz) {
          float4* dst = reinterpret_cast<float4*>(tuples + (size_t)eid * kGradFloats);
          dst[0] = make_float4(a[0], a[1], a[2], a[3]);
          dst[1] = make_float4(a[4], a[5], a[6], a[7]);
          dst[2] = make_float4(a[8], 0.f, 0.f, 0.f);
          flags[eid] = 1;
        }
      } else {
        float* dst = v_records + (size_t)gid * kGradFloats;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          if (a[c] != 0.f) {
            atomic_add_f32(dst + c, a[c]);
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (STATE) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      Tk[2 * h] = Tk2[h].x; Tk[2 * h + 1] = Tk2[h].y; Dv[2 * h] = Dv2[h].x; Dv[2 * h + 1] = Dv2[h].y;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = py0 + k;
      if (px < prm.W && y < prm.H) {
        size_t pix = ((size_t)s * prm.H + y) * prm.W + px;
        const float Tfin = out_T[pix];
        const float va_out = v_alpha ? v_alpha[pix] : 0.f;
        const float va = Tfin * (va_out - (bgr * vr[k] + bgg * vg[k] + bgb * vb[k]));
        bwd_T[pix] = Tk[k];
        bwd_B[pix] = Dv[k] + va;       // behind-colour . v_out
      }
    }
  }
}

#endif  // GS_ROUND1_KERNELS

// ---------------------------------------------------------------------------
// Backward compositor, scalar-cache variant (round 2; see raster.hip "scalar-cache variant" for the measurements
// behind it).  Same traversal and the same per-pixel recurrences as raster_bwd_kernel_v2, but
//   * the entry's record comes through the scalar cache (s_load_dwordx8 + s_load_dword) instead of a per-lane
//     gather + 12 v_readlane_b32 (7.9 cycles each); the list is walked backwards in aligned groups of four
//     entries, two register sets of two records each (one pair in flight while the other is processed);
//   * the five geometric gradients of a lane (x, y and the three conic terms) are built from THREE moments of
//     v_sigma over the lane's four pixels (sum w, sum w*dy, sum w*dy^2; dx is a lane constant): 4 packed ops per
//     pixel pair instead of 8, and 7 scalar ops per entry to expand them;
//   * a reduction group is the four entries of a list group; lanes 0..35 sum the 36 rows and store their total
//     STRAIGHT into the entry's gradient tuple (or atomically into v_records): no per-batch totals in LDS, no
//     per-batch flush, no vector loads of ids / records at all.
// LDS per wave: 36 rows x 36 floats = 5.1 KB (pair sums in registers first; 36 x 68 floats = 9.6 KB without).
// ---------------------------------------------------------------------------
struct RecS { float x, y, cx, cy, cz, op, r, g, b, nmid, kmul, qx, qz, d; };

// DEPTH: also the camera-space depth (record float 9), the fourth colour channel of the depth gradient
template <bool DEPTH>
__device__ __forceinline__ RecS load_rec_s(const float* __restrict__ records, unsigned gi) {
  const float* p = records + (size_t)gi * kRecFloats;
  RecS o;
  o.x = p[0]; o.y = p[1]; o.cx = p[2]; o.cy = p[3]; o.cz = p[4]; o.op = p[5]; o.r = p[6]; o.g = p[7]; o.b = p[8];
  o.nmid = p[kRecNmid]; o.kmul = p[kRecKmul]; o.qx = p[kRecQx]; o.qz = p[kRecQz];
  o.d = DEPTH ? p[9] : 0.f;
  return o;
}

constexpr int kRedG4 = 4;
// Horizontally adjacent lanes add their partial sums in registers (one DPP add per value) before the trip through
// LDS: 32 columns per row instead of 64 -> 5.1 KB of LDS per wave instead of 9.6 KB, so the occupancy limit moves
// from LDS (4 waves per SIMD) to the VGPRs (5), and the row sums read half as much.
constexpr int kRedCols4 = 32, kRedStride4 = 36;    // 36 = 32 + 4: rows 16-byte aligned, b128 row reads conflict-free
#ifndef GS_BWD_SLOAD_WAVES
#define GS_BWD_SLOAD_WAVES 5
#endif
constexpr int kRedFloats4 = kRedG4 * 9 * kRedStride4;
// the depth-gradient specialisation reduces a tenth row per entry: sum of weight * v_depth (tuple slot 11)
// the absgrad specialisations reduce two more rows per entry, BEFORE the depth row: the sums over the entry's pixels of
// |d loss / d x| and |d loss / d y| of each (pixel, Gaussian) pair (tuple slots 9 and 10), so that with both switches
// the depth row is row 11 = its tuple slot
constexpr int red_rows(bool depth, bool absgrad = false) { return 9 + (absgrad ? 2 : 0) + (depth ? 1 : 0); }
constexpr int red_floats(bool depth, bool absgrad = false) { return kRedG4 * red_rows(depth, absgrad) * kRedStride4; }

// w[i] = v[i](lane) + v[i](lane ^ 1) for nine values: nine v_add_f32_dpp in one block (the DPP combiner leaves most
// of them as v_mov_b32_dpp + v_add_f32 otherwise).  The s_nop covers the VALU-write -> DPP-read hazard, which the
// compiler's hazard recogniser cannot see inside inline assembly.
__device__ __forceinline__ void pair_sum9(float (&v)[9]) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %4, %4, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %5, %5, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %6, %6, %6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %7, %7, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %8, %8, %8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]));
}

// w = v(lane) + v(lane ^ 1) for one value (the tenth row of the depth specialisation; s_nop as in pair_sum9)
__device__ __forceinline__ void pair_sum1(float& v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(v));
}

// w = v(lane) + v(lane ^ 1) for two values (the absgrad rows; s_nop as in pair_sum9)
__device__ __forceinline__ void pair_sum2(float& a, float& b) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(a), "+v"(b));
}

// ---------------------------------------------------------------------------
// One list entry against the lane's four pixels (returns whether any lane of the wave was hit; then the lane's 9
// partial sums are in LDS rows slot*9 .. slot*9+8, column `lane >> 1`).
// Quadrant mapping (round 4): the lane's pixel k lies in the 8x8 quadrant (k & 1, k >> 1) of the tile (lane = (x8, y8)
// inside a quadrant) instead of four consecutive rows of one column as in the forward.  A splat of a few pixels reaches
// two or three of a tile's four quadrants (2.96 of 4 on the fitted-model-like scene, 3.7 on the benchmark scene:
// profiles/lane_stats.jsonl), and with this mapping "nobody's pixel k blended this entry" is a WAVE-UNIFORM fact: a
// quadrant without a hit is skipped by a scalar branch right after its validity test (two fma, two compares) — before
// the exp, the reciprocal and the ~20 multiply-adds of the gradient terms.  Measured against the column mapping, visit
// r4_v5: backward 4.33 vs 4.66 ms on the fitted-model-like scene, 0.70 vs 0.71 on the benchmark scene.  (An 8x8-tile
// BINNING would skip the same work but sort and reduce ~3x the entries)  dx takes two values per
// lane (left / right quadrants), so the moments of v_sigma are kept per column half: M0 and M1 twice, M2 once.
// Validity is the forward's ONE compare on the shifted exponent (raster.hip, gs_math.h rec_aux) on bit-identical
// operands (dx = x - pixel centre, never "left dx - 8"), so both directions take the same decision for every pixel and
// entry; alpha = kmul * 2^u; and because v_sigma = -alpha * v_alpha and v_opacity = (alpha / op) * v_alpha under the
// same gate, the opacity gradient is -(sum of v_sigma) / op: slot 5 carries RAW_OP ? the plain sum of v_sigma (the
// tuple reduce divides by -op once per Gaussian) : the finished gradient.
// CLAMP=false: no Gaussian of the tile's list has an opacity above 0.999 (tile_hot, see the forward).
// ---------------------------------------------------------------------------
// DEPTH (a depth gradient is present): the camera-space depth is a fourth colour channel with background 0 — the pixel's
// v_depth joins the colour dot product cv (so v_alpha and the behind-sum Dv carry it: no extra per-pixel state between
// slices) and the entry's tenth partial sum, sum of weight * v_depth, is d loss / d depth (tuple slot 11).
// ABSGRAD (the caller asked for xy_absgrad_out): the moments give the SIGNED sum of the centre gradient only, so the
// absolute values are taken per pixel, per component, before any summation: ax += |v_sigma * (cx dx + cy dy)|,
// ay += |v_sigma * (cy dx + cz dy)| (a pixel that is not hit has v_sigma = 0 and adds an exact zero).  |.| is a source
// modifier: the loop grows by four VALU per pixel (two fma for the bracket, two fma with |.| operands for the sums) and
// four multiplies per entry (cx dx, cy dx for both column halves).  Rows 9 and 10 = tuple slots 9 and 10.
struct BwdQuad { float T[4], Dv[4], vr[4], vg[4], vb[4], py[4], vd[4]; int fin[4]; };

template <bool CLAMP, bool RAW_OP, bool DEPTH, bool ABSGRAD = false>
__device__ __forceinline__ bool bwd_entry(const RecS& rc, float pxf, int idx, BwdQuad& pp, float* __restrict__ red,
                                          int slot, int lane, float agm) {
  // pxf: the lane's pixel-centre column in the LEFT quadrants; the right ones are 8 further (exact in fp32)
  const float dxa = rc.x - pxf, dxb = rc.x - (pxf + 8.0f);
  const float qyn = rc.cy * kNegLog2e;
  const float hx[2] = {fmaf(rc.qx * dxa, dxa, rc.nmid), fmaf(rc.qx * dxb, dxb, rc.nmid)};
  const float bx[2] = {qyn * dxa, qyn * dxb};
  float m0[2] = {0.f, 0.f}, m1[2] = {0.f, 0.f}, m2 = 0.f, q_r = 0.f, q_g = 0.f, q_b = 0.f, q_d = 0.f;
  float ax = 0.f, ay = 0.f;
  const float cxdx[2] = {rc.cx * dxa, rc.cx * dxb}, cydx[2] = {rc.cy * dxa, rc.cy * dxb};      // ABSGRAD only
  bool any = false;
  // (measured negatives, removed in round 6 — the records are in profiles/: the six per-entry record fields copied to
  //  VGPRs once per entry instead of 24 SGPR-operand uses; lanes that did not blend the entry sitting the body out under
  //  the exec mask instead of a selected alpha = 0: ISA 599 -> 607 VALU, 0.724 -> 0.737 ms, profiles/r05_exec_mask_ab.log)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dy = rc.y - pp.py[k];
    const float u = fmaf(dy, fmaf(rc.qz, dy, bx[k & 1]), hx[k & 1]);
    const bool hit = (idx < pp.fin[k]) && (fabsf(u) <= rc.nmid);
    if (__builtin_amdgcn_ballot_w64(hit) == 0ull) continue;           // nobody's quadrant-k pixel blended this entry
    any = true;
    const float ov = rc.kmul * __builtin_amdgcn_exp2f(u);
    // pixels that are not hit are neutralised by SELECTING alpha = 0 (1/(1-0) = 1 exactly, every term an exact zero)
    const float alpha = hit ? (CLAMP ? fminf(K::kAlphaMax, ov) : ov) : 0.f;
    const float ovm = CLAMP ? ((hit && ov <= agm) ? ov : 0.f) : alpha;   // d min(0.999, o*vis) = 0 when clamped
    const float ra = __builtin_amdgcn_rcpf(1.f - alpha);
    pp.T[k] *= ra;                               // transmittance in front of this Gaussian
    const float fac = alpha * pp.T[k];
    q_r = fmaf(fac, pp.vr[k], q_r); q_g = fmaf(fac, pp.vg[k], q_g); q_b = fmaf(fac, pp.vb[k], q_b);
    float cv = fmaf(rc.b, pp.vb[k], fmaf(rc.g, pp.vg[k], rc.r * pp.vr[k]));
    if (DEPTH) { q_d = fmaf(fac, pp.vd[k], q_d); cv = fmaf(rc.d, pp.vd[k], cv); }
    const float v_al = fmaf(pp.T[k], cv, -(ra * pp.Dv[k]));
    pp.Dv[k] = fmaf(fac, cv, pp.Dv[k]);
    const float v_sigma = -ovm * v_al;
    const float vsdy = v_sigma * dy;
    m0[k & 1] += v_sigma;
    m1[k & 1] += vsdy;
    m2 = fmaf(vsdy, dy, m2);
    if (ABSGRAD) {
      ax = fmaf(fabsf(v_sigma), fabsf(fmaf(rc.cy, dy, cxdx[k & 1])), ax);
      ay = fmaf(fabsf(v_sigma), fabsf(fmaf(rc.cz, dy, cydx[k & 1])), ay);
    }
  }
  if (!any) return false;
  // sum over the lane's pixels of v_sigma * {1, dx, dx^2} and of v_sigma * dy * {1, dx}
  const float M0 = m0[0] + m0[1], M1 = m1[0] + m1[1];
  const float X0 = fmaf(dxb, m0[1], dxa * m0[0]);                     // sum v_sigma dx
  const float X1 = fmaf(dxb, m1[1], dxa * m1[0]);                     // sum v_sigma dx dy
  const float XX = fmaf(dxb * dxb, m0[1], (dxa * dxa) * m0[0]);       // sum v_sigma dx^2
  const float p_cx = 0.5f * XX, p_cy = X1, p_cz = 0.5f * m2;
  const float p_x = fmaf(rc.cx, X0, rc.cy * M1);
  const float p_y = fmaf(rc.cy, X0, rc.cz * M1);
  const float p_op = RAW_OP ? M0 : -M0 * __builtin_amdgcn_rcpf(rc.op);
  float w[9] = {p_x, p_y, p_cx, p_cy, p_cz, p_op, q_r, q_g, q_b};
  pair_sum9(w);
  if (ABSGRAD) pair_sum2(ax, ay);
  if (DEPTH) pair_sum1(q_d);
  if ((lane & 1) == 0) {
    float* r0 = red + slot * (red_rows(DEPTH, ABSGRAD) * kRedStride4) + (lane >> 1);
#pragma unroll
    for (int c = 0; c < 9; ++c) r0[c * kRedStride4] = w[c];
    if (ABSGRAD) { r0[9 * kRedStride4] = ax; r0[10 * kRedStride4] = ay; }
    if (DEPTH) r0[(ABSGRAD ? 11 : 9) * kRedStride4] = q_d;
  }
  return true;
}

// the tile's list, back to front, entries [range_x, wave_end)
template <bool CLAMP, int OUT, bool DEPTH, bool ABSGRAD = false, class State>
__device__ __forceinline__ void bwd_walk(const int* __restrict__ ids, const int* __restrict__ eids,
                                         const float* __restrict__ records, unsigned max_id, int range_x, int wave_end,
                                         unsigned n, float pxf, float agm, State& pp, float* __restrict__ red,
                                         int lane, float* __restrict__ v_records, float* __restrict__ tuples,
                                         unsigned char* __restrict__ flags) {
  constexpr int kRows = red_rows(DEPTH, ABSGRAD);
  const int row = lane;                                    // row-sum role: lanes 0..35 (0..39 with DEPTH; ABSGRAD: 0..43 / 0..47)
  const int row_g = row / kRows, row_c = row - row_g * kRows;
  // tuple / gradient-record slot of the row (depth: 11; with ABSGRAD every row is its own slot, the depth row is row 11)
  const int slot_c = (DEPTH && !ABSGRAD && row_c == 9) ? 11 : row_c;
  const int4* __restrict__ ids4 = reinterpret_cast<const int4*>(ids);
  const int4* __restrict__ eids4 = reinterpret_cast<const int4*>(eids);
  int b = (wave_end - 1) & ~3;
  const int b_last = range_x & ~3;
  int4 idv = ids4[b >> 2];
  RecS a0 = load_rec_s<DEPTH>(records, min((unsigned)idv.w, max_id)), a1 = load_rec_s<DEPTH>(records, min((unsigned)idv.z, max_id));
  for (;;) {
    // pair A (entries b+3, b+2) is ready; put pair B (b+1, b) and the indices of the next (lower) group in flight
    asm volatile("" :: "s"(a0.x), "s"(a1.x) : "memory");
    const RecS b0 = load_rec_s<DEPTH>(records, min((unsigned)idv.y, max_id)), b1 = load_rec_s<DEPTH>(records, min((unsigned)idv.x, max_id));
    const int4 cur = idv;
    int4 ev = cur;
    if (OUT == 1) ev = eids4[b >> 2];
    // (unconditional: a conditional refill turns into a phi whose copies wait for the loads right where they are
    // issued; below the tile's first group the previous group — or group 0 again — is fetched and never used)
    idv = ids4[max(b - 4, 0) >> 2];
    asm volatile("" ::: "memory");
    unsigned filled = 0;
    if ((unsigned)(b + 3 - range_x) < n && bwd_entry<CLAMP, OUT == 1, DEPTH, ABSGRAD>(a0, pxf, b + 3, pp, red, 3, lane, agm)) filled |= 8u;
    if ((unsigned)(b + 2 - range_x) < n && bwd_entry<CLAMP, OUT == 1, DEPTH, ABSGRAD>(a1, pxf, b + 2, pp, red, 2, lane, agm)) filled |= 4u;
    // pair B is ready; refill pair A from the next group
    asm volatile("" :: "s"(b0.x), "s"(b1.x), "s"(idv.x), "s"(ev.x) : "memory");
    a0 = load_rec_s<DEPTH>(records, min((unsigned)idv.w, max_id)); a1 = load_rec_s<DEPTH>(records, min((unsigned)idv.z, max_id));
    asm volatile("" ::: "memory");
    if ((unsigned)(b + 1 - range_x) < n && bwd_entry<CLAMP, OUT == 1, DEPTH, ABSGRAD>(b0, pxf, b + 1, pp, red, 1, lane, agm)) filled |= 2u;
    if ((unsigned)(b - range_x) < n && bwd_entry<CLAMP, OUT == 1, DEPTH, ABSGRAD>(b1, pxf, b, pp, red, 0, lane, agm)) filled |= 1u;
    if (filled) {
      __builtin_amdgcn_wave_barrier();
      if (row < kRedG4 * kRows && ((filled >> row_g) & 1u)) {
        const f4* rp = reinterpret_cast<const f4*>(red + row * kRedStride4);
        f4 s0 = rp[0], s1 = rp[1], s2 = rp[2], s3 = rp[3];
#pragma unroll
        for (int q = 4; q < kRedCols4 / 4; q += 4) { s0 += rp[q]; s1 += rp[q + 1]; s2 += rp[q + 2]; s3 += rp[q + 3]; }
        const f4 v = (s0 + s1) + (s2 + s3);
        const float sum = (v.x + v.y) + (v.z + v.w);
        const int id_e = row_g == 0 ? ev.x : (row_g == 1 ? ev.y : (row_g == 2 ? ev.z : ev.w));
        if (OUT == 1) {
          tuples[(size_t)(unsigned)id_e * kGradFloats + slot_c] = sum;
          if (row_c == 0) flags[(unsigned)id_e] = 2;          // 2: slot 5 is the plain sum of v_sigma (see bwd_entry)
        } else {
          if (sum != 0.f) atomic_add_f32(v_records + (size_t)(unsigned)id_e * kGradFloats + slot_c, sum);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (b <= b_last) break;
    b -= 4;
  }
}

// per-pixel state accessors
__device__ __forceinline__ void pix_set(BwdQuad& st, int k, float T, float Dv, float vr, float vg, float vb, float py, int fin,
                                        float vd) {
  st.T[k] = T; st.Dv[k] = Dv; st.vr[k] = vr; st.vg[k] = vg; st.vb[k] = vb; st.py[k] = py; st.fin[k] = fin; st.vd[k] = vd;
}
__device__ __forceinline__ void pix_get(const BwdQuad& st, int k, float& T, float& Dv, float& vr, float& vg, float& vb) {
  T = st.T[k]; Dv = st.Dv[k]; vr = st.vr[k]; vg = st.vg[k]; vb = st.vb[k];
}
// raster_bwd_sload_kernel<STATE, OUT, DEPTH, ABSGRAD, CAMS>: ONE kernel template, the feature switches are template
// parameters of the kernel itself.
//   DEPTH   (gs_frame_backward_depth): v_depth [S,H,W] = d loss / d depth_acc, one more reduced row = tuple slot 11;
//   ABSGRAD (variant bit GS_BWD_ABSGRAD: the caller asked for xy_absgrad_out): two more reduced rows per entry, the sums
//           of |d loss / d x| and |d loss / d y| per (pixel, Gaussian) pair, in tuple slots 9 and 10 of EVERY flagged tuple;
//   CAMS    (frames of several cameras, gs_frame_desc.cameras > 1): sample image s belongs to camera s / s_cam, whose
//           combine scale is row block s / s_cam of cmb_scale [B,H,W,3].
// Why this form: a shared __device__ body changes these kernels' instruction streams (register allocation, branch
// shapes), which profiles/traffic.json's ISA hash, tests/test_occupancy.py and bench.py's roofline counters key on;
// template parameters on the kernel do not (profiles/kernel_templates_refactor.md).  v_depth and s_cam are ALWAYS
// present (nullptr, 1 when unused) so that every instantiation has one signature and one launch path.
template <bool STATE, int OUT, bool DEPTH = false, bool ABSGRAD = false, bool CAMS = false>
__global__ __launch_bounds__(256, GS_BWD_SLOAD_WAVES) void raster_bwd_sload_kernel(
    RasterParams prm, const int* __restrict__ ids /*record index per sorted entry, padded*/,
    const int* __restrict__ eids /*OUT==1: emission index per sorted entry (sorted_vals), padded*/,
    const float* __restrict__ records, unsigned max_id, const float* __restrict__ out_T,
    const int* __restrict__ final_idx, const float* __restrict__ v_img, const float* __restrict__ v_alpha,
    float* __restrict__ v_records, unsigned n_blocks, float* __restrict__ bwd_T, float* __restrict__ bwd_B,
    float* __restrict__ tuples, unsigned char* __restrict__ flags,
    const unsigned char* __restrict__ tile_hot, const float* __restrict__ v_depth, int s_cam) {
  __shared__ __attribute__((aligned(16))) float lds_all[4 * red_floats(DEPTH, ABSGRAD)];
  const int lane = lane_id();
  float* red = lds_all + (threadIdx.x >> 6) * red_floats(DEPTH, ABSGRAD);   // wave-private
  const int T = prm.tiles_x * prm.tiles_y;
  const unsigned work = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)(xcd_remap(blockIdx.x, n_blocks) * 4u + (threadIdx.x >> 6)));
  if (work >= (unsigned)(prm.S * T)) return;
  const int s = work / T, t = work % T;
  const int ty = t / prm.tiles_x, tx = t % prm.tiles_x;
  const int p = s * prm.R + find_band(prm.band_edges, prm.R, ty);
  int2 range = prm.tile_bins[(size_t)p * T + t];
  range.x = __builtin_amdgcn_readfirstlane(range.x);
  range.y = __builtin_amdgcn_readfirstlane(range.y);
  if (range.y <= range.x) return;

  // lane -> its four pixels, one per 8x8 quadrant: pixel k at (px0 + kx(k), py0 + ky(k))
  const int px0 = tx * K::kTile + (lane & 7);
  const int py0 = ty * K::kTile + (lane >> 3);
  auto kx = [](int k) { return 8 * (k & 1); };
  auto ky = [](int k) { return 8 * (k >> 1); };
  const float pxf = (float)px0 + 0.5f;
  const float bgr = prm.background[0], bgg = prm.background[1], bgb = prm.background[2];
  BwdQuad pp;
  int my_end = range.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = px0 + kx(k), y = py0 + ky(k);
    float Tk = 1.f, Dv = 0.f, vr = 0.f, vg = 0.f, vb = 0.f, vd = 0.f;
    int fin = range.x;
    if (x < prm.W && y < prm.H) {
      size_t pix = ((size_t)s * prm.H + y) * prm.W + x;
      const float Tfin = out_T[pix];
      fin = final_idx[pix];
      if (DEPTH) vd = v_depth[pix];
      vr = v_img[pix * 3 + 0]; vg = v_img[pix * 3 + 1]; vb = v_img[pix * 3 + 2];
      if (prm.cmb_scale) {
        const size_t q = ((CAMS ? (size_t)(s / s_cam) * prm.H + y : (size_t)y) * prm.W + x) * 3;
        vr = combine_grad(vr, prm.cmb_scale[q + 0], prm.cmb_gamma, prm.cmb_min);
        vg = combine_grad(vg, prm.cmb_scale[q + 1], prm.cmb_gamma, prm.cmb_min);
        vb = combine_grad(vb, prm.cmb_scale[q + 2], prm.cmb_gamma, prm.cmb_min);
      }
      const float va_out = v_alpha ? v_alpha[pix] : 0.f;
      const float va = Tfin * (va_out - (bgr * vr + bgg * vg + bgb * vb));
      Tk = Tfin;
      Dv = -va;
      if (STATE) {
        Tk = bwd_T[pix];
        Dv = bwd_B[pix] - va;
      }
    }
    my_end = max(my_end, fin);
    pix_set(pp, k, Tk, Dv, vr, vg, vb, (float)y + 0.5f, fin, vd);
  }
  const int wave_end = __builtin_amdgcn_readfirstlane(wave_max_i(my_end));
  const unsigned n = (unsigned)(wave_end - range.x);       // entries [range.x, wave_end) reached some pixel's final index
  const float agm = prm.alpha_grad_max;
  if (n != 0u) {
    const bool hot = tile_hot == nullptr || __builtin_amdgcn_readfirstlane((int)tile_hot[(size_t)p * T + t]) != 0;
    if (hot) bwd_walk<true, OUT, DEPTH, ABSGRAD>(ids, eids, records, max_id, range.x, wave_end, n, pxf, agm, pp, red, lane, v_records, tuples, flags);
    else bwd_walk<false, OUT, DEPTH, ABSGRAD>(ids, eids, records, max_id, range.x, wave_end, n, pxf, agm, pp, red, lane, v_records, tuples, flags);
  }
  if (STATE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = px0 + kx(k), y = py0 + ky(k);
      if (x < prm.W && y < prm.H) {
        float Tk, Dv, vr, vg, vb;
        pix_get(pp, k, Tk, Dv, vr, vg, vb);
        size_t pix = ((size_t)s * prm.H + y) * prm.W + x;
        const float Tfin = out_T[pix];
        const float va_out = v_alpha ? v_alpha[pix] : 0.f;
        const float va = Tfin * (va_out - (bgr * vr + bgg * vg + bgb * vb));
        bwd_T[pix] = Tk;
        bwd_B[pix] = Dv + va;       // behind-colour . v_out
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Splat-parallel backward (round 6; VERDICT round 5 item 2a: "build, not cost").  MEASURED NEGATIVE, kept selectable
// (variant bit 1024) so that the measurement can be repeated: profiles/r06_bwd_splat_parallel.md.
// Lane = one list entry of a 64-entry chunk (chunks back to front, lane 0 = the chunk's last entry); the tile's 256
// pixels stream through the wave as a systolic pipeline: at step s lane j works on pixel s - j, whose running state
// (transmittance in front, behind-colour . v_out) it takes over from lane j - 1 with two wave-wide DPP shifts — lane 0
// feeds pixel s from LDS, lane 63 hands pixel s - 63 back to LDS for the next chunk.  A lane accumulates ITS entry's
// nine sums over all 256 pixels in registers and stores the finished tuple itself: no cross-lane reduction, no LDS
// transpose, no tuple flags race.  What it pays: every (entry, pixel) pair costs a full evaluation — the tile-per-wave
// kernel above skips an entry with four wave-uniform quadrant tests when nobody blends it, and averages 64 VALU
// wave-instructions per entry on the fitted-model-like scene where this form needs ~60 per STEP, 319 steps per chunk.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float dpp_wave_shr1(float fresh_lane0, float v) {
  // lane j <- lane j - 1; lane 0 has no source and keeps `old` = the value fed into the pipeline (bound_ctrl off)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fresh_lane0), __float_as_int(v), 0x138 /*wave_shr:1*/,
                                                    0xf, 0xf, false));
}

template <bool STATE>
__global__ __launch_bounds__(256) void raster_bwd_splat_kernel(
    RasterParams prm, const int* __restrict__ ids, const int* __restrict__ eids, const float* __restrict__ records,
    unsigned max_id, const float* __restrict__ out_T, const int* __restrict__ final_idx, const float* __restrict__ v_img,
    const float* __restrict__ v_alpha, unsigned n_blocks, float* __restrict__ bwd_T, float* __restrict__ bwd_B,
    float* __restrict__ tuples, unsigned char* __restrict__ flags) {
  __shared__ float s_all[4][6][256];                       // per wave: vr, vg, vb, T, Dv, fin (int bits)
  const int lane = lane_id();
  float (*sp)[256] = s_all[threadIdx.x >> 6];
  const int T = prm.tiles_x * prm.tiles_y;
  const unsigned work = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)(xcd_remap(blockIdx.x, n_blocks) * 4u + (threadIdx.x >> 6)));
  if (work >= (unsigned)(prm.S * T)) return;
  const int s = work / T, t = work % T;
  const int ty = t / prm.tiles_x, tx = t % prm.tiles_x;
  const int p_sub = s * prm.R + find_band(prm.band_edges, prm.R, ty);
  int2 range = prm.tile_bins[(size_t)p_sub * T + t];
  range.x = __builtin_amdgcn_readfirstlane(range.x);
  range.y = __builtin_amdgcn_readfirstlane(range.y);
  if (range.y <= range.x) return;
  const float bgr = prm.background[0], bgg = prm.background[1], bgb = prm.background[2];
  int my_end = range.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int pidx = lane + 64 * q;
    const int x = tx * K::kTile + (pidx & 15), y = ty * K::kTile + (pidx >> 4);
    float Tk = 1.f, Dv = 0.f, vr = 0.f, vg = 0.f, vb = 0.f;
    int fin = range.x;
    if (x < prm.W && y < prm.H) {
      const size_t pix = ((size_t)s * prm.H + y) * prm.W + x;
      const float Tfin = out_T[pix];
      fin = final_idx[pix];
      vr = v_img[pix * 3 + 0]; vg = v_img[pix * 3 + 1]; vb = v_img[pix * 3 + 2];
      if (prm.cmb_scale) {
        const size_t qq = ((size_t)y * prm.W + x) * 3;
        vr = combine_grad(vr, prm.cmb_scale[qq + 0], prm.cmb_gamma, prm.cmb_min);
        vg = combine_grad(vg, prm.cmb_scale[qq + 1], prm.cmb_gamma, prm.cmb_min);
        vb = combine_grad(vb, prm.cmb_scale[qq + 2], prm.cmb_gamma, prm.cmb_min);
      }
      const float va_out = v_alpha ? v_alpha[pix] : 0.f;
      const float va = Tfin * (va_out - (bgr * vr + bgg * vg + bgb * vb));
      Tk = Tfin;
      Dv = -va;
      if (STATE) { Tk = bwd_T[pix]; Dv = bwd_B[pix] - va; }
    }
    my_end = max(my_end, fin);
    sp[0][pidx] = vr; sp[1][pidx] = vg; sp[2][pidx] = vb; sp[3][pidx] = Tk; sp[4][pidx] = Dv;
    sp[5][pidx] = __int_as_float(fin);
  }
  const int wave_end = __builtin_amdgcn_readfirstlane(wave_max_i(my_end));
  const float agm = prm.alpha_grad_max;
  const float x0f = (float)(tx * K::kTile) + 0.5f, y0f = (float)(ty * K::kTile) + 0.5f;
  __builtin_amdgcn_wave_barrier();
  for (int e_hi = wave_end - 1; e_hi >= range.x; e_hi -= 64) {
    const int e = e_hi - lane;
    const bool active = e >= range.x;
    const unsigned gi = active ? min((unsigned)ids[e], max_id) : 0u;
    const float4* rp = reinterpret_cast<const float4*>(records + (size_t)gi * kRecFloats);
    const float4 ra4 = rp[0], rb4 = rp[1], rc4 = rp[2], rd4 = rp[3];
    const float gx = ra4.x, gy = ra4.y, cx = ra4.z, cy = ra4.w, cz = rb4.x, cr = rb4.z, cg = rb4.w, cb = rc4.x;
    const float nmid = active ? rd4.x : -1.f, kmul = rd4.y, qx = rd4.z, qz = rd4.w;    // nmid < 0: never valid
    const float qyn = cy * kNegLog2e;
    float M0 = 0.f, X0 = 0.f, Y0 = 0.f, XX = 0.f, XY = 0.f, YY = 0.f, q_r = 0.f, q_g = 0.f, q_b = 0.f;
    bool touched = false;
    float Tp = 0.f, Dp = 0.f;                                  // the pipeline registers of this lane
    asm volatile("" ::: "memory");
#pragma unroll 1
    for (int st = 0; st < 256 + 63; ++st) {
      const int feed = min(st, 255);
      Tp = dpp_wave_shr1(sp[3][feed], Tp);
      Dp = dpp_wave_shr1(sp[4][feed], Dp);
      const int pidx = st - lane;
      const bool inp = (unsigned)pidx < 256u;
      const int pc = inp ? pidx : 0;
      const float vr = sp[0][pc], vg = sp[1][pc], vb = sp[2][pc];
      const int fin = __float_as_int(sp[5][pc]);
      const float dx = gx - (x0f + (float)(pc & 15)), dy = gy - (y0f + (float)(pc >> 4));
      // the forward's validity expression, operand for operand (raster.hip blend_entry)
      const float hx = fmaf(qx * dx, dx, nmid), bx = qyn * dx;
      const float u = fmaf(dy, fmaf(qz, dy, bx), hx);
      const bool hit = inp && (e < fin) && (fabsf(u) <= nmid);
      const float ov = kmul * __builtin_amdgcn_exp2f(u);
      const float alpha = hit ? fminf(K::kAlphaMax, ov) : 0.f;
      const float ovm = (hit && ov <= agm) ? ov : 0.f;
      const float ra = __builtin_amdgcn_rcpf(1.f - alpha);
      Tp *= ra;
      const float fac = alpha * Tp;
      q_r = fmaf(fac, vr, q_r); q_g = fmaf(fac, vg, q_g); q_b = fmaf(fac, vb, q_b);
      const float cv = fmaf(cb, vb, fmaf(cg, vg, cr * vr));
      const float v_al = fmaf(Tp, cv, -(ra * Dp));
      Dp = fmaf(fac, cv, Dp);
      const float v_sigma = -ovm * v_al;
      const float vsx = v_sigma * dx, vsy = v_sigma * dy;
      M0 += v_sigma; X0 += vsx; Y0 += vsy;
      XX = fmaf(vsx, dx, XX); XY = fmaf(vsx, dy, XY); YY = fmaf(vsy, dy, YY);
      touched |= hit;
      if (lane == 63 && inp) { sp[3][pidx] = Tp; sp[4][pidx] = Dp; }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (active && touched) {
      const size_t slot = (size_t)(unsigned)eids[e];
      float4* dst = reinterpret_cast<float4*>(tuples + slot * kGradFloats);
      dst[0] = make_float4(fmaf(cx, X0, cy * Y0), fmaf(cy, X0, cz * Y0), 0.5f * XX, XY);
      dst[1] = make_float4(0.5f * YY, M0, q_r, q_g);
      dst[2] = make_float4(q_b, 0.f, 0.f, 0.f);
      flags[slot] = 2;                                          // slot 5: the plain sum of v_sigma
    }
  }
  if (STATE) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pidx = lane + 64 * q;
      const int x = tx * K::kTile + (pidx & 15), y = ty * K::kTile + (pidx >> 4);
      if (x < prm.W && y < prm.H) {
        const size_t pix = ((size_t)s * prm.H + y) * prm.W + x;
        const float Tfin = out_T[pix];
        const float va_out = v_alpha ? v_alpha[pix] : 0.f;
        const float va = Tfin * (va_out - (bgr * sp[0][pidx] + bgg * sp[1][pidx] + bgb * sp[2][pidx]));
        bwd_T[pix] = sp[3][pidx];
        bwd_B[pix] = sp[4][pidx] + va;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Segmented sum of the gradient tuples of one depth slice.  The tuples of slice Gaussian j occupy
// [cum[j], cum[j]+counts[j]) (emission order); flags mark the entries the backward actually touched.
// A wave owns 64 Gaussians: short segments are summed by their own lane, long ones (near Gaussians
// cover hundreds of tiles) by the whole wave with one DPP reduction per component.  Every Gaussian
// belongs to exactly one slice, so the result is a plain store into v_records — no atomics anywhere.
// ---------------------------------------------------------------------------
constexpr unsigned kReduceSolo = 16;
constexpr int kTupleComp = 11;
// DEPTH: a twelfth component, slot 11 = d loss / d depth (the depth specialisations of the compositors write it)
constexpr int tuple_comp(bool depth) { return depth ? 12 : kTupleComp; }

template <bool DEPTH>
__device__ __forceinline__ void reduce_tuples_body(int n_slice, const unsigned* __restrict__ slice_gi,
                                                            const unsigned* __restrict__ counts,
                                                            const unsigned* __restrict__ cum,
                                                            const float* __restrict__ tuples,
                                                            const unsigned char* __restrict__ flags,
                                                            float* __restrict__ v_records,
                                                            unsigned char* __restrict__ touched,
                                                            const float* __restrict__ records, unsigned mult) {
  const int lane = lane_id();
  const int j = blockIdx.x * 256 + threadIdx.x;
  unsigned cnt = 0, e0 = 0, gi = 0;
  // mult: tuples per list entry (gs_rasterize_bwd_rs_slice with one list for S samples writes S of them, adjacent)
  if (j < n_slice) { cnt = counts[j] * mult; e0 = cum[j] * mult; gi = slice_gi[j]; }
  // 11 components: slots 9 and 10 carry d loss / d pixel-velocity of the exact rolling-shutter compositor
  // (raster_rs.hip), or the absgrad sums of the SE(3) compositors' absgrad instantiations (every flagged tuple of such a
  // launch has both written); the other compositors leave them unwritten and nobody reads their sums
  constexpr int kComp = tuple_comp(DEPTH);
  float acc[kComp];
#pragma unroll
  for (int c = 0; c < kComp; ++c) acc[c] = 0.f;
  bool any = false, raw = false;     // raw: slot 5 holds the plain sum of v_sigma (flag value 2)
  if (cnt && cnt <= kReduceSolo) {
    for (unsigned i = 0; i < cnt; ++i) {
      const unsigned char f = flags[e0 + i];
      if (f) {
        const float4* t = reinterpret_cast<const float4*>(tuples + (size_t)(e0 + i) * kGradFloats);
        float4 a = t[0], b = t[1], c = t[2];
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
        acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w; acc[8] += c.x; acc[9] += c.y; acc[10] += c.z;
        if (DEPTH) acc[kComp - 1] += c.w;
        any = true;
        raw |= f == 2;
      }
    }
  }
  unsigned long long big = __ballot(cnt > kReduceSolo);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const unsigned c_n = (unsigned)readlane_i((int)cnt, src), c_e = (unsigned)readlane_i((int)e0, src);
    float part[kComp];
#pragma unroll
    for (int c = 0; c < kComp; ++c) part[c] = 0.f;
    bool hit = false, hraw = false;
    for (unsigned i = lane; i < c_n; i += 64) {
      const unsigned char f = flags[c_e + i];
      if (f) {
        const float4* t = reinterpret_cast<const float4*>(tuples + (size_t)(c_e + i) * kGradFloats);
        float4 a = t[0], b = t[1], c = t[2];
        part[0] += a.x; part[1] += a.y; part[2] += a.z; part[3] += a.w;
        part[4] += b.x; part[5] += b.y; part[6] += b.z; part[7] += b.w; part[8] += c.x; part[9] += c.y; part[10] += c.z;
        if (DEPTH) part[kComp - 1] += c.w;
        hit = true;
        hraw |= f == 2;
      }
    }
    if (__ballot(hit) != 0ull) {
#pragma unroll
      for (int c = 0; c < kComp; ++c) {
        const float tsum = wave_sum_uniform(part[c]);
        if (lane == src) acc[c] = tsum;
      }
      const bool wraw = __ballot(hraw) != 0ull;
      if (lane == src) { any = true; raw = wraw; }
    }
  }
  if (any) {
    // slot 5 of the scalar-cache compositor's tuples is the plain sum of v_sigma: v_opacity = -sum / opacity
    if (raw) acc[5] *= -__builtin_amdgcn_rcpf(records[(size_t)gi * kRecFloats + 5]);
    float4* dst = reinterpret_cast<float4*>(v_records + (size_t)gi * kGradFloats);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    dst[2] = make_float4(acc[8], acc[9], acc[10], DEPTH ? acc[kComp - 1] : 0.f);
    if (touched) touched[gi] = 1;
  }
}

// wave-per-Gaussian form for slices of few, large Gaussians (the nearest slice: ~50k Gaussians owning
// ~400 tiles each): the thread-per-Gaussian form would run 200 blocks with 64-deep serial ballot loops.
template <bool DEPTH>
__device__ __forceinline__ void reduce_tuples_wave_body(int n_slice, const unsigned* __restrict__ slice_gi,
                                                                 const unsigned* __restrict__ counts,
                                                                 const unsigned* __restrict__ cum,
                                                                 const float* __restrict__ tuples,
                                                                 const unsigned char* __restrict__ flags,
                                                                 float* __restrict__ v_records,
                                                                 unsigned char* __restrict__ touched,
                                                                 const float* __restrict__ records, unsigned mult) {
  const int lane = lane_id();
  const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (j >= n_slice) return;
  const unsigned c_n = counts[j] * mult, c_e = cum[j] * mult;
  if (c_n == 0) return;
  constexpr int kComp = tuple_comp(DEPTH);
  float part[kComp];
#pragma unroll
  for (int c = 0; c < kComp; ++c) part[c] = 0.f;
  bool hit = false, hraw = false;
  for (unsigned i = lane; i < c_n; i += 64) {
    const unsigned char f = flags[c_e + i];
    if (f) {
      const float4* t = reinterpret_cast<const float4*>(tuples + (size_t)(c_e + i) * kGradFloats);
      float4 a = t[0], b = t[1], c = t[2];
      part[0] += a.x; part[1] += a.y; part[2] += a.z; part[3] += a.w;
      part[4] += b.x; part[5] += b.y; part[6] += b.z; part[7] += b.w; part[8] += c.x; part[9] += c.y; part[10] += c.z;
      if (DEPTH) part[kComp - 1] += c.w;
      hit = true;
      hraw |= f == 2;
    }
  }
  if (__ballot(hit) == 0ull) return;
  const bool raw = __ballot(hraw) != 0ull;
  float tot[kComp];
#pragma unroll
  for (int c = 0; c < kComp; ++c) tot[c] = wave_sum_uniform(part[c]);
  if (lane == 0) {
    const unsigned gi = slice_gi[j];
    if (raw) tot[5] *= -__builtin_amdgcn_rcpf(records[(size_t)gi * kRecFloats + 5]);
    float4* dst = reinterpret_cast<float4*>(v_records + (size_t)gi * kGradFloats);
    dst[0] = make_float4(tot[0], tot[1], tot[2], tot[3]);
    dst[1] = make_float4(tot[4], tot[5], tot[6], tot[7]);
    dst[2] = make_float4(tot[8], tot[9], tot[10], DEPTH ? tot[kComp - 1] : 0.f);
    if (touched) touched[gi] = 1;
  }
}

__global__ __launch_bounds__(256) void reduce_tuples_kernel(
    int n_slice, const unsigned* __restrict__ slice_gi, const unsigned* __restrict__ counts,
    const unsigned* __restrict__ cum, const float* __restrict__ tuples, const unsigned char* __restrict__ flags,
    float* __restrict__ v_records, unsigned char* __restrict__ touched, const float* __restrict__ records, unsigned mult) {
  reduce_tuples_body<false>(n_slice, slice_gi, counts, cum, tuples, flags, v_records, touched, records, mult);
}
__global__ __launch_bounds__(256) void reduce_tuples_wave_kernel(
    int n_slice, const unsigned* __restrict__ slice_gi, const unsigned* __restrict__ counts,
    const unsigned* __restrict__ cum, const float* __restrict__ tuples, const unsigned char* __restrict__ flags,
    float* __restrict__ v_records, unsigned char* __restrict__ touched, const float* __restrict__ records, unsigned mult) {
  reduce_tuples_wave_body<false>(n_slice, slice_gi, counts, cum, tuples, flags, v_records, touched, records, mult);
}
// the depth forms (slot 11 summed as well)
__global__ __launch_bounds__(256) void reduce_tuples_depth_kernel(
    int n_slice, const unsigned* __restrict__ slice_gi, const unsigned* __restrict__ counts,
    const unsigned* __restrict__ cum, const float* __restrict__ tuples, const unsigned char* __restrict__ flags,
    float* __restrict__ v_records, unsigned char* __restrict__ touched, const float* __restrict__ records, unsigned mult) {
  reduce_tuples_body<true>(n_slice, slice_gi, counts, cum, tuples, flags, v_records, touched, records, mult);
}
__global__ __launch_bounds__(256) void reduce_tuples_wave_depth_kernel(
    int n_slice, const unsigned* __restrict__ slice_gi, const unsigned* __restrict__ counts,
    const unsigned* __restrict__ cum, const float* __restrict__ tuples, const unsigned char* __restrict__ flags,
    float* __restrict__ v_records, unsigned char* __restrict__ touched, const float* __restrict__ records, unsigned mult) {
  reduce_tuples_wave_body<true>(n_slice, slice_gi, counts, cum, tuples, flags, v_records, touched, records, mult);
}

}  // namespace gs

using namespace gs;

// Replaces _C.rasterize_backward: one pass over complete tile lists.  v_records must be
// zeroed by the caller; gradients are accumulated with fp32 atomics (the gsplat-compatible op has no
// emission-order index to build tuples from).  n_records > 0: scalar-cache kernel (sorted_vals padded by 8 ints).
GS_EXPORT int gs_rasterize_bwd(const float* records, const int* sorted_vals, const int* tile_bins,
                               const int* band_edges, const float* background, int S, int R, int H, int W,
                               const float* out_T, const int* final_idx, const float* v_img, const float* v_alpha,
                               float* v_records, int n_records, int variant, void* stream) {
  if (S <= 0 || R <= 0 || H <= 0 || W <= 0) return GS_ERR_INVALID;
  RasterParams prm = make_raster_params(records, sorted_vals, tile_bins, band_edges, background, S, R, H, W);
  if (variant & GS_VARIANT_CLAMP_GRAD) { prm.alpha_grad_max = 3.0e38f; variant &= ~GS_VARIANT_CLAMP_GRAD; }
  const unsigned work = (unsigned)(S * prm.tiles_x * prm.tiles_y), blocks = (work + 3) / 4;
  const dim3 grid(blocks), block(256);
  float* const no_f = nullptr;
  unsigned char* const no_u8 = nullptr;
  if (variant == 0) {
    if (n_records == 0) return GS_OK;       // not a single list entry: no gradient (v_records stays zero)
    if (n_records > 0) {
      hipLaunchKernelGGL((raster_bwd_sload_kernel<false, 0>), grid, block, 0, (hipStream_t)stream, prm, sorted_vals,
                         sorted_vals, records, (unsigned)(n_records - 1), out_T, final_idx, v_img, v_alpha, v_records,
                         blocks, no_f, no_f, no_f, no_u8, (const unsigned char*)nullptr, (const float*)nullptr, 1);
      return gs_launch_status();
    }
  }
#if GS_ROUND1_KERNELS
  hipLaunchKernelGGL((raster_bwd_kernel_v2<false, 0>), grid, block, 0, (hipStream_t)stream, prm, out_T, final_idx, v_img,
                     v_alpha, v_records, blocks, no_f, no_f, no_f, no_u8);
  return gs_launch_status();
#else
  return GS_ERR_INVALID;      // the round-1 backward is not in this build
#endif
}

// One backward launch per slice, slices back to front.  bwd_T (initialised by the caller to out_T) and
// bwd_B [S,H,W] (behind-colour . v_out, initialised to 0) carry the reverse-traversal state between launches.
// gs_rasterize_bwd_slice_depth (library-internal: gs_internal.h, called by csrc/frame.hip) also takes
//   v_depth [S,H,W] = d loss / d depth_acc: non-NULL selects the depth specialisations (tuple slot 11 = d loss / d depth);
//   cameras > 1 (a frame of several cameras, S = cameras * samples per camera) with cmb_scale [cameras,H,W,3]: the
//     camera-indexed instantiations.  Without cmb_scale (v_img holds the per-sample gradients) the count changes nothing;
//   variant bit GS_BWD_ABSGRAD: the absgrad instantiations, which also write tuple slots 9 and 10 of every flagged tuple.
// Which combinations run which kernel, and which are refused, is the ONE rule block below.
extern "C" int gs_rasterize_bwd_slice_depth(const float* records, const int* sorted_vals, const int* tile_bins,
                                            const int* band_edges, const float* background, int S, int R, int H, int W,
                                            const float* out_T, const int* final_idx, const float* v_img,
                                            const float* v_alpha, float* bwd_T, float* bwd_B, float* v_records,
                                            const int* gi_of_e, float* tuples, unsigned char* flags,
                                            const int* sorted_ids, int n_records, const unsigned char* tile_hot,
                                            int variant, const float* cmb_scale, float cmb_gamma, float cmb_min_level,
                                            const float* v_depth, int cameras, void* stream) {
  if (S <= 0 || R <= 0 || H <= 0 || W <= 0) return GS_ERR_INVALID;
  RasterParams prm = make_raster_params(records, sorted_vals, tile_bins, band_edges, background, S, R, H, W);
  prm.gi_of_e = gi_of_e;
  prm.cmb_scale = cmb_scale; prm.cmb_gamma = cmb_gamma; prm.cmb_min = cmb_min_level;
  if (variant & GS_VARIANT_CLAMP_GRAD) { prm.alpha_grad_max = 3.0e38f; variant &= ~GS_VARIANT_CLAMP_GRAD; }
  const unsigned work = (unsigned)(S * prm.tiles_x * prm.tiles_y), blocks = (work + 3) / 4;
  const dim3 grid(blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  // scalar-cache kernels: record index per sorted entry = sorted_ids, or sorted_vals itself when it holds Gaussian ids
  const int* ids = sorted_ids ? sorted_ids : (gi_of_e ? nullptr : sorted_vals);
  const unsigned max_id = (unsigned)(n_records > 0 ? n_records - 1 : 0);

  const bool tup = tuples && flags && gi_of_e;        // tuple form (no atomics); otherwise v_records is accumulated into
  const bool state = bwd_T && bwd_B;                  // reverse-traversal state of a frame of several slices
  const bool sload = n_records > 0 && ids;            // the scalar-cache kernels can run
  const bool absgrad = (variant & GS_BWD_ABSGRAD) != 0, depth = v_depth != nullptr, cams = cameras > 1 && cmb_scale;
  // a null state pair reaches the STATE = false instantiations as null
  float* const bT = state ? bwd_T : nullptr;
  float* const bB = state ? bwd_B : nullptr;
  // every instantiation of raster_bwd_sload_kernel has one signature, so there is one argument list
  auto launch = [&](auto* kernel, const int* eids, int s_cam) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, prm, ids, eids, records, max_id, out_T, final_idx, v_img, v_alpha,
                       v_records, blocks, bT, bB, tuples, flags, tile_hot, v_depth, s_cam);
    return gs_launch_status();
  };
  // the tuple-form instantiation <STATE, 1, DEPTH, ABSGRAD, CAMS> of the four runtime switches (a runtime bool becomes a
  // template argument through std::integral_constant)
  auto with = [](bool b, auto f) { return b ? f(std::true_type{}) : f(std::false_type{}); };
  auto tuple_kernel = [&] {
    return with(state, [&](auto s_) { return with(depth, [&](auto d_) { return with(absgrad, [&](auto a_) {
      return with(cams, [&](auto c_) { return raster_bwd_sload_kernel<s_.value, 1, d_.value, a_.value, c_.value>; });
    }); }); });
  };

  // ---- the dispatch rule (GS_VARIANT_CLAMP_GRAD is stripped above) --------------------------------------------------
  if (!tup && !state) return GS_ERR_INVALID;          // the atomic form exists with state only
  if (absgrad || depth || cams) {
    // the specialised instantiations {absgrad} x {depth} x {cams}: scalar-cache kernels in tuple form only.  variant is
    // GS_BWD_ABSGRAD or 0 and nothing else — except that the splat-parallel bit (no depth channel, no absgrad) is
    // tolerated and IGNORED with a depth gradient and no absgrad: the depth kernel runs
    if (depth && !absgrad) variant &= ~GS_VARIANT_SPLAT;
    if (variant != (absgrad ? GS_BWD_ABSGRAD : 0) || !sload || !tup || (cams && S % cameras != 0)) return GS_ERR_INVALID;
    return launch(tuple_kernel(), sorted_vals, cams ? S / cameras : 1);   // sample image s belongs to camera s / s_cam
  }
  if (variant == 0 && sload) {
    if (tup) return launch(tuple_kernel(), sorted_vals, 1);     // no state: the only slice
    return launch(raster_bwd_sload_kernel<true, 0>, ids, 1);    // atomic form
  }
  if (variant == GS_VARIANT_SPLAT && sload && tup) {
    // the splat-parallel formulation (measurement only: see raster_bwd_splat_kernel)
    hipLaunchKernelGGL(state ? raster_bwd_splat_kernel<true> : raster_bwd_splat_kernel<false>, grid, block, 0, st, prm,
                       ids, sorted_vals, records, max_id, out_T, final_idx, v_img, v_alpha, blocks, bT, bB, tuples, flags);
    return gs_launch_status();
  }
#if GS_ROUND1_KERNELS
  // everything else (GS_VARIANT_ROUND1, or no record-index list): the round-1 kernel, tuple or atomic form
  hipLaunchKernelGGL((!tup ? raster_bwd_kernel_v2<true, 0> : state ? raster_bwd_kernel_v2<true, 1> : raster_bwd_kernel_v2<false, 1>),
                     grid, block, 0, st, prm, out_T, final_idx, v_img, v_alpha, v_records, blocks, bT, bB, tuples, flags);
  return gs_launch_status();
#else
  return GS_ERR_INVALID;        // the round-1 backward (GS_VARIANT_ROUND1, or no record-index list) is not in this build
#endif
}

GS_EXPORT int gs_rasterize_bwd_slice(const float* records, const int* sorted_vals, const int* tile_bins,
                                     const int* band_edges, const float* background, int S, int R, int H, int W,
                                     const float* out_T, const int* final_idx, const float* v_img,
                                     const float* v_alpha, float* bwd_T, float* bwd_B, float* v_records,
                                     const int* gi_of_e, float* tuples, unsigned char* flags,
                                     const int* sorted_ids, int n_records, const unsigned char* tile_hot,
                                     int variant, const float* cmb_scale, float cmb_gamma, float cmb_min_level,
                                     void* stream) {
  return gs_rasterize_bwd_slice_depth(records, sorted_vals, tile_bins, band_edges, background, S, R, H, W, out_T,
                                      final_idx, v_img, v_alpha, bwd_T, bwd_B, v_records, gi_of_e, tuples, flags,
                                      sorted_ids, n_records, tile_hot, variant, cmb_scale, cmb_gamma, cmb_min_level,
                                      nullptr, 1, stream);
}

// Sum each slice Gaussian's gradient tuples (written by gs_rasterize_bwd_slice with tuples != NULL) into
// v_records[slice_gi[j]] (plain stores; Gaussians without a touched entry are left as they are).
// flags[e] == 2 marks tuples of gs_rasterize_bwd_slice's scalar-cache kernel, whose slot 5 is the plain sum of v_sigma:
// the reduce turns it into the opacity gradient, -sum / records[gi].opacity (flags[e] == 1: slot 5 already is the
// opacity gradient — gs_rasterize_bwd_rs_slice, the round-1 kernel).
// gs_reduce_grad_tuples_depth (library-internal: gs_internal.h): depth != 0 also sums slot 11 (d loss / d depth, written
// by the depth specialisations of the compositors) into v_records[gi][11]; without it that slot is stored as 0.
extern "C" int gs_reduce_grad_tuples_depth(int n_slice, const unsigned* slice_gi, const unsigned* counts,
                                           const unsigned* cum_excl, const float* tuples, const unsigned char* flags,
                                           float* v_records, unsigned char* touched, long long n_isect,
                                           const float* records, int tuples_per_entry, int depth, void* stream) {
  if (n_slice <= 0 || !records || tuples_per_entry < 1) return GS_ERR_INVALID;
  // the kernels index tuples and flags with 32-bit (entry * tuples_per_entry) offsets
  if (n_isect > 0 && n_isect * (long long)tuples_per_entry >= 4294967296ll) return GS_ERR_INVALID;
  const unsigned mult = (unsigned)tuples_per_entry;
  // few large Gaussians (n_isect > 32 * n_slice): one wave each; otherwise one thread each
  const bool wave = n_isect > 32ll * n_slice;
  const auto kernel = wave ? (depth ? reduce_tuples_wave_depth_kernel : reduce_tuples_wave_kernel)
                           : (depth ? reduce_tuples_depth_kernel : reduce_tuples_kernel);
  hipLaunchKernelGGL(kernel, dim3(wave ? (n_slice + 3) / 4 : (n_slice + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     n_slice, slice_gi, counts, cum_excl, tuples, flags, v_records, touched, records, mult);
  return gs_launch_status();
}

GS_EXPORT int gs_reduce_grad_tuples(int n_slice, const unsigned* slice_gi, const unsigned* counts,
                                    const unsigned* cum_excl, const float* tuples, const unsigned char* flags,
                                    float* v_records, unsigned char* touched, long long n_isect, const float* records,
                                    int tuples_per_entry, void* stream) {
  return gs_reduce_grad_tuples_depth(n_slice, slice_gi, counts, cum_excl, tuples, flags, v_records, touched, n_isect,
                                     records, tuples_per_entry, 0, stream);
}

