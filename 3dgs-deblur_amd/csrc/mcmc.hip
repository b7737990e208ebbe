// mcmc.hip — the two kernels of the 3DGS-MCMC strategy (mcmc.py): the opacity-gated noise that follows EVERY optimizer
// step, and the opacity / scale correction of relocated Gaussians.  Math: mcmc_math.h.  gfx950, wave64.
#include "gs_common.h"
#include "mcmc_math.h"

namespace {

// One thread per Gaussian, grid-stride.  Per row: one 16-byte load (the quaternion) and ten dwords (log-scales, logit,
// means in / out; rows of 12 bytes are not 16-byte aligned, neighbouring lanes share their cache lines) = 56 bytes.
// No row is skipped: where the gate underflows to 0 the update is means + 0, which a skip would reproduce except for a
// mean of -0.0f (-0 + 0 = +0) and for non-finite covariances — so every row takes the same path.
template <bool NOISE_IN, bool NOISE_OUT>
__global__ __launch_bounds__(256) void mcmc_inject_noise_kernel(int N, float* __restrict__ means,
                                                                 const float* __restrict__ log_scales,
                                                                 const float4* __restrict__ quats,
                                                                 const float* __restrict__ logits, float scaler,
                                                                 unsigned long long seed, unsigned long long step,
                                                                 const float* __restrict__ noise_in,
                                                                 float* __restrict__ noise_out) {
  const int stride = (int)gridDim.x * 256;
  for (int r = (int)blockIdx.x * 256 + (int)threadIdx.x; r < N; r += stride) {
    const size_t r3 = (size_t)r * 3;
    const float4 qv = quats[r];
    const float q[4] = {qv.x, qv.y, qv.z, qv.w};
    const float ls[3] = {log_scales[r3], log_scales[r3 + 1], log_scales[r3 + 2]};
    const float logit = logits[r];
    float m[3] = {means[r3], means[r3 + 1], means[r3 + 2]};
    float z[3];
    if (NOISE_IN) {
      z[0] = noise_in[r3]; z[1] = noise_in[r3 + 1]; z[2] = noise_in[r3 + 2];
    } else {
      uint32_t w[4];
      gs::mcmc::row_words((uint32_t)r, seed, step, w);
      gs::mcmc::normals3(w, z);
    }
    if (NOISE_OUT) {
      noise_out[r3] = z[0]; noise_out[r3 + 1] = z[1]; noise_out[r3 + 2] = z[2];
    }
    float d[3];
    gs::mcmc::noise_delta(ls, q, logit, z, scaler, d);
    means[r3] = m[0] + d[0];
    means[r3 + 1] = m[1] + d[1];
    means[r3 + 2] = m[2] + d[2];
  }
}

// one thread per sampled row
__global__ __launch_bounds__(256) void mcmc_relocation_kernel(int M, const float* __restrict__ opacities,
                                                               const float* __restrict__ scales,
                                                               const int* __restrict__ ratios,
                                                               float* __restrict__ new_opacities,
                                                               float* __restrict__ new_scales) {
  const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= M) return;
  const size_t r3 = (size_t)r * 3;
  const float s[3] = {scales[r3], scales[r3 + 1], scales[r3 + 2]};
  float o, ns[3];
  gs::mcmc::relocation(opacities[r], s, ratios[r], &o, ns);
  new_opacities[r] = o;
  new_scales[r3] = ns[0]; new_scales[r3 + 1] = ns[1]; new_scales[r3 + 2] = ns[2];
}

}  // namespace

// see include/gsdeblur.h
GS_EXPORT int gs_mcmc_inject_noise(int N, float* means, const float* log_scales, const float* quats,
                                   const float* opacity_logits, float scaler, long long seed, long long step,
                                   const float* noise_in, float* noise_out, void* stream) {
  if (N < 0) return GS_ERR_INVALID;
  if (N == 0) return GS_OK;
  if (!means || !log_scales || !quats || !opacity_logits) return GS_ERR_INVALID;
  if ((uintptr_t)quats & 15) return GS_ERR_INVALID;            // the quaternion rows are read as 16-byte loads
  // the grid follows the 16-byte loads of the launch (one per row, 256 per block), capped at 8 blocks per CU of the
  // 256 CUs; the rows beyond that are reached by the grid stride
  const long long want = ((long long)N + 255) / 256;
  const unsigned blocks = (unsigned)(want > 2048 ? 2048 : want);
  const float4* q4 = reinterpret_cast<const float4*>(quats);
  const unsigned long long sd = (unsigned long long)seed, stp = (unsigned long long)step;
  hipStream_t st = (hipStream_t)stream;
#define GS_MCMC_LAUNCH(NI, NO)                                                                                     \
  hipLaunchKernelGGL((mcmc_inject_noise_kernel<NI, NO>), dim3(blocks), dim3(256), 0, st, N, means, log_scales, q4, \
                     opacity_logits, scaler, sd, stp, noise_in, noise_out)
  if (noise_in) {
    if (noise_out) GS_MCMC_LAUNCH(true, true); else GS_MCMC_LAUNCH(true, false);
  } else {
    if (noise_out) GS_MCMC_LAUNCH(false, true); else GS_MCMC_LAUNCH(false, false);
  }
#undef GS_MCMC_LAUNCH
  return gs_launch_status();
}

// see include/gsdeblur.h
GS_EXPORT int gs_mcmc_relocation(int M, const float* opacities, const float* scales, const int* ratios,
                                 float* new_opacities, float* new_scales, void* stream) {
  if (M < 0) return GS_ERR_INVALID;
  if (M == 0) return GS_OK;
  if (!opacities || !scales || !ratios || !new_opacities || !new_scales) return GS_ERR_INVALID;
  const unsigned blocks = (unsigned)(((long long)M + 255) / 256);
  hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, M, opacities, scales,
                     ratios, new_opacities, new_scales);
  return gs_launch_status();
}
