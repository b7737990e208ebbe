// normals.hip — normals from the rendered depth, normal-prior and normal smoothness loss (normals.py): from the
// compositor's per-sample sums depth_acc, alphas [B,S,H,W] and the camera's intrinsics to normals [B,H,W,3], the loss per
// frame and d loss / d depth_acc, d loss / d alphas.  Math: normal_math.h.  gfx950, wave64.
//
// A workgroup of kThreads = kTileW * kTileH threads takes kGroupTiles tiles of kTileW x kTileH pixels next to each other in
// x, one after the other, one pixel per thread; what it needs around a tile sits in LDS.  Two launches, nothing is read
// back between them:
//   1. forward: the 2 S planes are read once per pixel over tile + 2 rings and reduced to the sample means d, a; normals on
//      tile + 1 ring; the tile's normals are stored, and (d, a) are stashed as one float2 per pixel (DESIGN 5.15 says why);
//      every thread adds the prior term of its pixel and the pairs its pixel owns (q = p + x, p + y) to six float64 sums,
//      which sums_loss.h's block_add adds (butterfly, then the waves in wave order): one record per workgroup;
//   2. gradient: the same grid.  Every workgroup first adds its frame's records (sums_loss.h frame_sum: thread t records
//      t, t + kThreads, ... in order, then block_add, so all workgroups of a frame hold the same bits) and derives the
//      coefficients; per tile it loads (d, a) and the stored normals over tile + 2 rings, rebuilds v_n, v_tx, v_ty on
//      tile + 1 ring (float64, in LDS), gathers v_z for its pixel and stores the 2 S gradient planes.  Workgroup 0 of a
//      frame also stores loss[b] and stats[b][6].
// gs_depth_normals is launch 1 without the sums and the stash.  No atomics; the order of every sum depends on H and W
// alone, so two runs agree bit for bit and a frame's result does not depend on what else is in the batch.
#include "sums_loss.h"
#include "normal_math.h"

namespace {

namespace nm = gs::normal;
namespace dp = gs::depthprior;
namespace sums = gs::sums;

constexpr int kTileW = 32;
constexpr int kTileH = 8;
constexpr int kGroupTiles = 8;                    // tiles per workgroup: 1080 workgroups and records for a 1080p frame
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / gs::kWave;
constexpr int kHaloW = kTileW + 4, kHaloH = kTileH + 4;      // tile + 2 rings
constexpr int kRingW = kTileW + 2, kRingH = kTileH + 2;      // tile + 1 ring

static_assert(kThreads == kTileW * kTileH && kThreads % gs::kWave == 0 && nm::kStats <= kThreads, "layout");
static_assert(sizeof(nm::Sums) == nm::kStats * sizeof(double), "records are 6 doubles");

struct Frame {
  int S, H, W, groups_x;
  float min_alpha, edge_beta;
};

// launch 1.  kLoss = false: normals only (records, stash, prior and guide are not touched)
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void normal_fwd_kernel(Frame f, const float* __restrict__ depth_acc,
                                                               const float* __restrict__ alphas,
                                                               const float* __restrict__ intrins,
                                                               const float* __restrict__ prior,
                                                               const float* __restrict__ guide,
                                                               double* __restrict__ records, float2* __restrict__ stash,
                                                               float* __restrict__ normals) {
  __shared__ float sd[kHaloW * kHaloH], sa[kHaloW * kHaloH];
  __shared__ float sn[kRingW * kRingH * 3];
  __shared__ double wave_part[kWaves * nm::kStats];
  __shared__ double part[nm::kStats];
  const int t = (int)threadIdx.x, b = (int)blockIdx.y;
  const int gx = (int)blockIdx.x % f.groups_x, y0 = ((int)blockIdx.x / f.groups_x) * kTileH;
  const int H = f.H, W = f.W, S = f.S;
  const size_t pixels = (size_t)H * (size_t)W, frame = (size_t)b * (size_t)S * pixels, image = (size_t)b * pixels;
  const float K[4] = {intrins[b * 4 + 0], intrins[b * 4 + 1], intrins[b * 4 + 2], intrins[b * 4 + 3]};
  nm::Sums m;
  nm::clear_sums(m);
  for (int k = 0; k < kGroupTiles; ++k) {
    const int x0 = (gx * kGroupTiles + k) * kTileW;
    if (x0 >= W) break;                                     // the same for every thread
    __syncthreads();                                        // the tile before is done with the LDS arrays
    for (int i = t; i < kHaloW * kHaloH; i += kThreads) {
      const int u = x0 - 2 + i % kHaloW, v = y0 - 2 + i / kHaloW;
      float d = 0.0f, a = 0.0f;
      if (u >= 0 && u < W && v >= 0 && v < H) {
        const size_t p = (size_t)v * W + u;
        d = dp::sample_mean(depth_acc + frame + p, pixels, S);
        a = dp::sample_mean(alphas + frame + p, pixels, S);
      }
      sd[i] = d;
      sa[i] = a;
    }
    __syncthreads();
    for (int i = t; i < kRingW * kRingH; i += kThreads) {
      const int rx = i % kRingW, ry = i / kRingW, h = (ry + 1) * kHaloW + rx + 1;
      float n[3];
      nm::normal_at(sd + h, sa + h, kHaloW, x0 - 1 + rx, y0 - 1 + ry, H, W, K, f.min_alpha, n);
      sn[i * 3 + 0] = n[0]; sn[i * 3 + 1] = n[1]; sn[i * 3 + 2] = n[2];
    }
    __syncthreads();
    const int lx = t % kTileW, ly = t / kTileW, u = x0 + lx, v = y0 + ly;
    if (u < W && v < H) {
      const size_t p = (size_t)v * W + u;
      const int r = (ly + 1) * kRingW + lx + 1, h = (ly + 2) * kHaloW + lx + 2;
      const float n[3] = {sn[r * 3 + 0], sn[r * 3 + 1], sn[r * 3 + 2]};
      float* out = normals + (image + p) * 3;
      out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
      if (kLoss) {
        stash[image + p] = make_float2(sd[h], sa[h]);
        if (nm::defined(n)) {
          nm::add_defined(m);
          float unit[3];
          if (prior && nm::prior_unit(prior + (image + p) * 3, unit)) nm::add_prior(m, n, unit);
          const float* nr = sn + (r + 1) * 3;                // a normal right of or below the frame does not exist
          const float* nd = sn + (r + kRingW) * 3;
          if (nm::defined(nr)) nm::add_pair(m, n, nr, guide ? nm::pair_weight(guide + (image + p) * 3, guide + (image + p + 1) * 3, f.edge_beta) : 1.0f);
          if (nm::defined(nd)) nm::add_pair(m, n, nd, guide ? nm::pair_weight(guide + (image + p) * 3, guide + (image + p + W) * 3, f.edge_beta) : 1.0f);
        }
      }
    }
  }
  if (kLoss) {
    sums::block_add<kWaves>(m, wave_part, part);
    if (t < nm::kStats) records[((size_t)b * gridDim.x + blockIdx.x) * nm::kStats + t] = part[t];
  }
}

// launch 2
__global__ __launch_bounds__(kThreads) void normal_grad_kernel(Frame f, float prior_weight, float smooth_weight,
                                                                const float2* __restrict__ stash,
                                                                const float* __restrict__ normals,
                                                                const float* __restrict__ intrins,
                                                                const float* __restrict__ prior,
                                                                const float* __restrict__ guide,
                                                                const double* __restrict__ records,
                                                                float* __restrict__ loss, double* __restrict__ stats,
                                                                float* __restrict__ v_depth_acc,
                                                                float* __restrict__ v_alphas) {
  __shared__ float sd[kHaloW * kHaloH], sa[kHaloW * kHaloH];
  __shared__ float sn[kHaloW * kHaloH * 3];
  __shared__ double svt[kRingW * kRingH * 6];                // v_tx, v_ty
  __shared__ double wave_part[kWaves * nm::kStats];
  __shared__ double part[nm::kStats];
  const int t = (int)threadIdx.x, b = (int)blockIdx.y, groups = (int)gridDim.x;
  const int gx = (int)blockIdx.x % f.groups_x, y0 = ((int)blockIdx.x / f.groups_x) * kTileH;
  const int H = f.H, W = f.W, S = f.S;
  const size_t pixels = (size_t)H * (size_t)W, frame = (size_t)b * (size_t)S * pixels, image = (size_t)b * pixels;
  const float K[4] = {intrins[b * 4 + 0], intrins[b * 4 + 1], intrins[b * 4 + 2], intrins[b * 4 + 3]};
  const nm::Sums m = sums::frame_sum<kThreads>(reinterpret_cast<const nm::Sums*>(records) + (size_t)b * groups, groups,
                                              wave_part, part);
  const nm::Coef c = nm::finish(m, (double)prior_weight, (double)smooth_weight);
  if (blockIdx.x == 0 && t == 0) {
    loss[b] = (float)c.loss;
    double* st = stats + (size_t)b * nm::kStats;
    st[0] = m.n_def; st[1] = m.np; st[2] = m.sp; st[3] = m.ns; st[4] = m.ss; st[5] = m.sg;
  }
  for (int k = 0; k < kGroupTiles; ++k) {
    const int x0 = (gx * kGroupTiles + k) * kTileW;
    if (x0 >= W) break;
    __syncthreads();
    for (int i = t; i < kHaloW * kHaloH; i += kThreads) {
      const int u = x0 - 2 + i % kHaloW, v = y0 - 2 + i / kHaloW;
      float2 da = make_float2(0.0f, 0.0f);
      float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
      if (u >= 0 && u < W && v >= 0 && v < H) {
        const size_t p = image + (size_t)v * W + u;
        da = stash[p];
        n0 = normals[p * 3 + 0]; n1 = normals[p * 3 + 1]; n2 = normals[p * 3 + 2];
      }
      sd[i] = da.x; sa[i] = da.y;
      sn[i * 3 + 0] = n0; sn[i * 3 + 1] = n1; sn[i * 3 + 2] = n2;
    }
    __syncthreads();
    for (int i = t; i < kRingW * kRingH; i += kThreads) {
      const int rx = i % kRingW, ry = i / kRingW, h = (ry + 1) * kHaloW + rx + 1;
      const int u = x0 - 1 + rx, v = y0 - 1 + ry;
      const float* n = sn + h * 3;
      double vtx[3] = {0.0, 0.0, 0.0}, vty[3] = {0.0, 0.0, 0.0};
      if (nm::defined(n)) {                                  // an interior pixel of the frame: its neighbours are inside
        const size_t p = image + (size_t)v * W + u;
        float unit[3] = {0.0f, 0.0f, 0.0f};
        if (prior) nm::prior_unit(prior + p * 3, unit);
        double pair_sum[3] = {0.0, 0.0, 0.0};
        auto add_neighbour = [&](int hq, size_t q) {        // left, right, upper, lower: the order of the sum
          const float* nq = sn + hq * 3;
          if (!nm::defined(nq)) return;
          const float g = guide ? nm::pair_weight(guide + p * 3, guide + q * 3, f.edge_beta) : 1.0f;
          pair_sum[0] += (double)g * (double)nq[0]; pair_sum[1] += (double)g * (double)nq[1]; pair_sum[2] += (double)g * (double)nq[2];
        };
        add_neighbour(h - 1, p - 1);
        add_neighbour(h + 1, p + 1);
        add_neighbour(h - kHaloW, p - (size_t)W);
        add_neighbour(h + kHaloW, p + (size_t)W);
        double vn[3];
        nm::grad_normal(c, unit, pair_sum, vn);
        nm::Geom g;
        nm::geometry(u, v, K, sd[h - 1] / sa[h - 1], sd[h + 1] / sa[h + 1], sd[h - kHaloW] / sa[h - kHaloW],
                     sd[h + kHaloW] / sa[h + kHaloW], g);
        nm::grad_tangents(g, n, vn, vtx, vty);
      }
      double* o = svt + i * 6;
      o[0] = vtx[0]; o[1] = vtx[1]; o[2] = vtx[2]; o[3] = vty[0]; o[4] = vty[1]; o[5] = vty[2];
    }
    __syncthreads();
    const int lx = t % kTileW, ly = t / kTileW, u = x0 + lx, v = y0 + ly;
    if (u < W && v < H) {
      const size_t p = (size_t)v * W + u;
      const int r = (ly + 1) * kRingW + lx + 1, h = (ly + 2) * kHaloW + lx + 2;
      const float d = sd[h], a = sa[h];
      float vd = 0.0f, va = 0.0f;
      if (nm::has_z(d, a, f.min_alpha)) {
        const double* l = svt + (r - 1) * 6;
        const double* rr = svt + (r + 1) * 6;
        const double* up = svt + (r - kRingW) * 6 + 3;
        const double* dn = svt + (r + kRingW) * 6 + 3;
        const double vP[3] = {((l[0] - rr[0]) + up[0]) - dn[0], ((l[1] - rr[1]) + up[1]) - dn[1], ((l[2] - rr[2]) + up[2]) - dn[2]};
        dp::chain(nm::grad_z(u, v, K, vP), d, a, dp::kDepth, S, &vd, &va);
      }
      sums::store_pair(v_depth_acc, v_alphas, frame, pixels, p, S, vd, va);
    }
  }
}

int groups_x_of(int W) { return (W + kTileW * kGroupTiles - 1) / (kTileW * kGroupTiles); }
int groups_of(int H, int W) { return groups_x_of(W) * ((H + kTileH - 1) / kTileH); }

long long records_bytes(int B, int H, int W) { return (long long)B * groups_of(H, W) * (long long)sizeof(nm::Sums); }
long long stash_bytes(int B, int H, int W) { return (long long)B * H * W * (long long)sizeof(float2); }

}  // namespace

// see include/gsdeblur.h
GS_EXPORT int gs_depth_normals(int B, int S, int H, int W, const float* depth_acc, const float* alphas,
                               const float* intrins, float min_alpha, float* normals_out, void* stream) {
  if (!sums::shape_ok(B, S, H, W) || !(min_alpha >= 0.0f)) return GS_ERR_INVALID;
  if (B == 0) return GS_OK;
  if (!depth_acc || !alphas || !intrins || !normals_out) return GS_ERR_INVALID;
  const Frame f = {S, H, W, groups_x_of(W), min_alpha, 0.0f};
  hipLaunchKernelGGL(normal_fwd_kernel<false>, dim3((unsigned)groups_of(H, W), (unsigned)B), dim3(kThreads), 0,
                     (hipStream_t)stream, f, depth_acc, alphas, intrins, (const float*)nullptr, (const float*)nullptr,
                     (double*)nullptr, (float2*)nullptr, normals_out);
  return gs_launch_status();
}

// see include/gsdeblur.h
GS_EXPORT long long gs_normal_loss_workspace_bytes(int B, int S, int H, int W) {
  if (!sums::shape_ok(B, S, H, W)) return -1;
  return records_bytes(B, H, W) + stash_bytes(B, H, W) + (long long)B * H * W * 3 * (long long)sizeof(float);
}

// see include/gsdeblur.h
GS_EXPORT int gs_normal_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas, const float* intrins,
                             const float* prior, const float* guide, float prior_weight, float smooth_weight,
                             float edge_beta, float min_alpha, float* loss_out, double* stats_out, float* normals_out,
                             float* v_depth_acc, float* v_alphas, void* ws, long long ws_bytes, void* stream) {
  if (!sums::shape_ok(B, S, H, W)) return GS_ERR_INVALID;
  if (!(min_alpha >= 0.0f) || !(edge_beta >= 0.0f) || !(prior_weight == prior_weight) || !(smooth_weight == smooth_weight))
    return GS_ERR_INVALID;
  if (B == 0) return GS_OK;
  if (!intrins) return GS_ERR_INVALID;
  const int ok = sums::check_loss_call(depth_acc, alphas, loss_out, stats_out, v_depth_acc, v_alphas, ws, ws_bytes,
                                       gs_normal_loss_workspace_bytes(B, S, H, W));
  if (ok != GS_OK) return ok;
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(ws);
  double* records = reinterpret_cast<double*>(base);
  float2* stash = reinterpret_cast<float2*>(base + records_bytes(B, H, W));
  float* normals = normals_out ? normals_out : reinterpret_cast<float*>(base + records_bytes(B, H, W) + stash_bytes(B, H, W));
  if (!(edge_beta > 0.0f)) guide = nullptr;                 // g = 1
  const Frame f = {S, H, W, groups_x_of(W), min_alpha, edge_beta};
  const dim3 grid((unsigned)groups_of(H, W), (unsigned)B);
  hipLaunchKernelGGL(normal_fwd_kernel<true>, grid, dim3(kThreads), 0, st, f, depth_acc, alphas, intrins, prior, guide,
                     records, stash, normals);
  const int status = gs_launch_status();
  if (status != GS_OK) return status;
  hipLaunchKernelGGL(normal_grad_kernel, grid, dim3(kThreads), 0, st, f, prior_weight, smooth_weight, stash, normals, intrins,
                     prior, guide, records, loss_out, stats_out, v_depth_acc, v_alphas);
  return gs_launch_status();
}
