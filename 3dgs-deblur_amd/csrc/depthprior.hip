// depthprior.hip — scale- and shift-invariant depth-prior loss (depthprior.py): from the compositor's per-sample sums
// depth_acc, alphas [B,S,H,W] and a prior [B,H,W] to the loss per frame and d loss / d depth_acc, d loss / d alphas.
// Math: depthprior_math.h.  gfx950, wave64.
//
// Two launches, nothing is read back between them:
//   1. moments: grid (tiles of kTile pixels, B).  Thread t takes pixels t, t + kThreads, ... of its tile: the 2 S planes
//      and the prior are read plane-wise, coalesced.  The threads' seven float64 moments are added by sums_loss.h's
//      block_add (butterfly, then the waves in wave order) and stored: one record per tile;
//   2. gradient: the same grid.  Every workgroup first adds its frame's records (sums_loss.h frame_sum: thread t records
//      t, t + kThreads, ... in order, then block_add, so all workgroups of a frame hold the same bits), derives the float64
//      coefficients, RE-READS the 2 S planes of its tile (DESIGN 5.13 says why they are not stashed) and stores the 2 S
//      gradient planes.  Workgroup 0 of a frame also stores loss[b] and stats[b][8].
// No atomics; the order of every sum depends on H * W alone, so two runs agree bit for bit and a frame's result does not
// depend on what else is in the batch.
#include "sums_loss.h"
#include "depthprior_math.h"

namespace {

namespace dp = gs::depthprior;
namespace sums = gs::sums;

constexpr int kThreads = 256;
constexpr int kTile = 4096;                       // pixels per workgroup: 16 per thread, 507 tiles for a 1080p frame
constexpr int kWaves = kThreads / gs::kWave;

static_assert(kTile % kThreads == 0 && kThreads % gs::kWave == 0 && dp::kMoments <= kThreads, "layout");
static_assert(sizeof(dp::Moments) == dp::kMoments * sizeof(double), "records are 7 doubles");

// records [B][tiles][kMoments]
__global__ __launch_bounds__(kThreads) void depth_prior_moments_kernel(int S, int pixels, int tiles, int kind, int space,
                                                                        float min_alpha,
                                                                        const float* __restrict__ depth_acc,
                                                                        const float* __restrict__ alphas,
                                                                        const float* __restrict__ prior,
                                                                        double* __restrict__ records) {
  __shared__ double wave_part[kWaves * dp::kMoments];
  __shared__ double part[dp::kMoments];
  const int t = (int)threadIdx.x, tile = (int)blockIdx.x, b = (int)blockIdx.y;
  const size_t frame = (size_t)b * (size_t)S * (size_t)pixels;
  dp::Moments m;
  dp::clear_moments(m);
#pragma unroll 4
  for (int k = 0; k < kTile / kThreads; ++k) {
    const int p = tile * kTile + k * kThreads + t;
    if (p < pixels) {
      const float d = dp::sample_mean(depth_acc + frame + p, (size_t)pixels, S);
      const float a = dp::sample_mean(alphas + frame + p, (size_t)pixels, S);
      const float y = prior[(size_t)b * pixels + p];
      float x;
      const bool valid = dp::pixel_x(d, a, y, space, min_alpha, &x);
      dp::add_pixel(m, valid, x, y, kind);
    }
  }
  sums::block_add<kWaves>(m, wave_part, part);
  if (t < dp::kMoments) records[((size_t)b * tiles + tile) * dp::kMoments + t] = part[t];
}

__global__ __launch_bounds__(kThreads) void depth_prior_grad_kernel(int S, int pixels, int tiles, int kind, int space,
                                                                     float min_alpha, float weight,
                                                                     const float* __restrict__ depth_acc,
                                                                     const float* __restrict__ alphas,
                                                                     const float* __restrict__ prior,
                                                                     const double* __restrict__ records,
                                                                     float* __restrict__ loss, double* __restrict__ stats,
                                                                     float* __restrict__ v_depth_acc,
                                                                     float* __restrict__ v_alphas) {
  __shared__ double wave_part[kWaves * dp::kMoments];
  __shared__ double part[dp::kMoments];
  const int t = (int)threadIdx.x, tile = (int)blockIdx.x, b = (int)blockIdx.y;
  const dp::Moments m = sums::frame_sum<kThreads>(reinterpret_cast<const dp::Moments*>(records) + (size_t)b * tiles, tiles,
                                                 wave_part, part);
  const dp::Coef c = dp::finish(m, kind, (double)weight);
  if (tile == 0 && t == 0) {
    loss[b] = (float)c.loss;
    double* st = stats + (size_t)b * dp::kStats;
    st[0] = m.n; st[1] = m.sx; st[2] = m.sy; st[3] = m.sxx; st[4] = m.syy; st[5] = m.sxy; st[6] = m.sabs; st[7] = c.rho;
  }
  const size_t frame = (size_t)b * (size_t)S * (size_t)pixels;
#pragma unroll 4
  for (int k = 0; k < kTile / kThreads; ++k) {
    const int p = tile * kTile + k * kThreads + t;
    if (p < pixels) {
      const float d = dp::sample_mean(depth_acc + frame + p, (size_t)pixels, S);
      const float a = dp::sample_mean(alphas + frame + p, (size_t)pixels, S);
      const float y = prior[(size_t)b * pixels + p];
      float x, vd = 0.0f, va = 0.0f;
      if (dp::pixel_x(d, a, y, space, min_alpha, &x) && !c.degenerate) dp::chain(dp::grad_x(c, x, y), d, a, space, S, &vd, &va);
      sums::store_pair(v_depth_acc, v_alphas, frame, (size_t)pixels, (size_t)p, S, vd, va);
    }
  }
}

int tiles_of(long long pixels) { return (int)((pixels + kTile - 1) / kTile); }

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_depth_prior_workspace_bytes(int B, int S, int H, int W) {
  if (!sums::shape_ok(B, S, H, W)) return -1;
  return (long long)B * tiles_of((long long)H * W) * (long long)sizeof(dp::Moments);
}

// see include/gsdeblur.h
GS_EXPORT int gs_depth_prior_loss(int B, int S, int H, int W, const float* depth_acc, const float* alphas,
                                  const float* prior, int kind, int space, float min_alpha, float weight, float* loss_out,
                                  double* stats_out, float* v_depth_acc, float* v_alphas, void* ws, long long ws_bytes,
                                  void* stream) {
  if (!sums::shape_ok(B, S, H, W)) return GS_ERR_INVALID;
  if ((kind != dp::kPearson && kind != dp::kL1) || (space != dp::kDepth && space != dp::kDisparity)) return GS_ERR_INVALID;
  if (!(min_alpha >= 0.0f) || !(weight == weight)) return GS_ERR_INVALID;
  if (B == 0) return GS_OK;
  if (!prior) return GS_ERR_INVALID;
  const int ok = sums::check_loss_call(depth_acc, alphas, loss_out, stats_out, v_depth_acc, v_alphas, ws, ws_bytes,
                                       gs_depth_prior_workspace_bytes(B, S, H, W));
  if (ok != GS_OK) return ok;
  const int pixels = H * W, tiles = tiles_of(pixels);
  hipStream_t st = (hipStream_t)stream;
  double* records = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)tiles, (unsigned)B);
  hipLaunchKernelGGL(depth_prior_moments_kernel, grid, dim3(kThreads), 0, st, S, pixels, tiles, kind, space, min_alpha,
                     depth_acc, alphas, prior, records);
  const int status = gs_launch_status();
  if (status != GS_OK) return status;
  hipLaunchKernelGGL(depth_prior_grad_kernel, grid, dim3(kThreads), 0, st, S, pixels, tiles, kind, space, min_alpha, weight,
                     depth_acc, alphas, prior, records, loss_out, stats_out, v_depth_acc, v_alphas);
  return gs_launch_status();
}
