// sums_loss.h — what the loss kernels on the compositor's per-sample sums share (depthprior.hip, normals.hip; Python
// counterpart: _sums.py): the shape limits, the deterministic reduction of float64 records, the store of a pixel's gradient
// pair and the entry points' common checks.  For the two .hip files only; the math headers do not depend on it.
//
// A record is a struct of N doubles whose combination is the member-wise sum (depthprior_math.h add_moments,
// normal_math.h add_sums).  The order of every addition is fixed by the thread layout alone: no atomics.
#pragma once
#include "gs_common.h"

namespace gs {
namespace sums {

constexpr int kMaxPlanes = 256;                   // B * S
constexpr long long kMaxElems = 1LL << 30;        // B * S * H * W stays below it

inline bool shape_ok(int B, int S, int H, int W) {
  if (B < 0 || S < 1 || H < 1 || W < 1) return false;
  if ((long long)B * S > kMaxPlanes) return false;
  const long long pixels = (long long)H * W;
  return pixels < kMaxElems && (long long)(B > 0 ? B : 1) * S * pixels < kMaxElems;
}

template <class Record>
struct Doubles {
  static_assert(sizeof(Record) % sizeof(double) == 0, "records are doubles");
  static constexpr int kN = (int)(sizeof(Record) / sizeof(double));
  double v[kN];
};

// every thread's record -> the workgroup's, in part[0 .. N) (valid after the call for every thread): a butterfly over the
// 64 lanes, lane 0 of each wave leaves its N doubles in wave_part[kWaves * N], thread k < N adds the waves' member k in
// wave order
template <int kWaves, class Record>
__device__ __forceinline__ void block_add(const Record& record, double* wave_part, double* part) {
  constexpr int N = Doubles<Record>::kN;
  Doubles<Record> a = __builtin_bit_cast(Doubles<Record>, record);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Doubles<Record> b;                            // all N shuffles are issued before the first addition waits for one
#pragma unroll
    for (int k = 0; k < N; ++k) b.v[k] = __shfl_xor(a.v[k], o);
#pragma unroll
    for (int k = 0; k < N; ++k) a.v[k] += b.v[k];
  }
  const int t = (int)threadIdx.x;
  if (gs::lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) wave_part[(t / gs::kWave) * N + k] = a.v[k];
  }
  __syncthreads();
  if (t < N) {
    double sum = wave_part[t];
    for (int w = 1; w < kWaves; ++w) sum += wave_part[w * N + t];
    part[t] = sum;
  }
  __syncthreads();
}

// the sum of a frame's `count` records, the same bits in every thread of every workgroup that asks: thread t adds records
// t, t + kThreads, ... in order, then block_add
template <int kThreads, class Record>
__device__ __forceinline__ Record frame_sum(const Record* records, int count, double* wave_part, double* part) {
  constexpr int N = Doubles<Record>::kN;
  Doubles<Record> a;
#pragma unroll
  for (int k = 0; k < N; ++k) a.v[k] = 0.0;
  for (int r = (int)threadIdx.x; r < count; r += kThreads) {
    const Doubles<Record> b = __builtin_bit_cast(Doubles<Record>, records[r]);
#pragma unroll
    for (int k = 0; k < N; ++k) a.v[k] += b.v[k];
  }
  block_add<kThreads / gs::kWave>(__builtin_bit_cast(Record, a), wave_part, part);
#pragma unroll
  for (int k = 0; k < N; ++k) a.v[k] = part[k];
  return __builtin_bit_cast(Record, a);
}

// one pixel's gradient pair into its S planes of v_depth_acc and v_alphas; frame: the frame's first element, plane: the
// elements of a plane, p: the pixel in its plane
__device__ __forceinline__ void store_pair(float* v_depth_acc, float* v_alphas, size_t frame, size_t plane, size_t p, int S,
                                           float vd, float va) {
  for (int s = 0; s < S; ++s) {
    v_depth_acc[frame + (size_t)s * plane + p] = vd;
    v_alphas[frame + (size_t)s * plane + p] = va;
  }
}

// what the loss entry points check alike once B > 0: the common pointers, the alignment of the float64 arrays, the workspace
inline int check_loss_call(const void* depth_acc, const void* alphas, const void* loss_out, const void* stats_out,
                           const void* v_depth_acc, const void* v_alphas, const void* ws, long long ws_bytes,
                           long long ws_needed) {
  if (!depth_acc || !alphas || !loss_out || !stats_out || !v_depth_acc || !v_alphas || !ws) return GS_ERR_INVALID;
  if (((uintptr_t)ws & 7) || ((uintptr_t)stats_out & 7)) return GS_ERR_INVALID;
  return ws_bytes < ws_needed ? GS_ERR_WORKSPACE : GS_OK;
}

}  // namespace sums
}  // namespace gs
