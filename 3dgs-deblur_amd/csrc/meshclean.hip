// meshclean.hip — connected components of a triangle mesh and the removal of small ones (meshclean.py).  The graph, the
// rounds, the ranking and the survivor rule: meshclean_math.h.  gfx950, wave64.  Integers only: atomicMin, integer
// atomicAdd (exact, so every result is the same bits whatever the schedule), no float atomics, no CAS loop, and no
// workgroup waits on another.
//
// ROUNDS     one round = hook (one thread per face) + compress (one thread per vertex), two launches.  A hooking
//   workgroup stamps counts[kHookedRound] with the round's number once; the caller reads that word back and stops at the
//   first round that left it behind.  Inside a launch a thread may read a parent that another thread has replaced in the
//   meantime (L1 is per CU and not refreshed): it then sees an older ancestor of the same component (meshclean_math.h:
//   why that is harmless); the launch boundary publishes every store to the next kernel.
// FINISH     faces and vertices per root by integer atomicAdd (one add per wave where the wave's lanes agree on the root,
//   which is the rule on a mesh with one large component), the roots compacted in ascending order by an exclusive scan
//   of the root flags (gs_exclusive_scan_u32, reduce-then-scan), the table (root, faces, vertices) per component.
// PLAN       one workgroup finds the key of the keep_largest-th component by an 8 x 8-bit radix select over the table and
//   flags every root; keep flags per vertex and face, scanned to output positions; V', F', C, kept and the status word
//   wait in counts for one read-back.
// EMIT       one launch: surviving vertices (with colours) and re-indexed faces at their positions.
#include "gs_common.h"
#include "meshclean_math.h"

namespace {

namespace mc = gs::meshclean;

constexpr int kBlock = 256;
constexpr int kSelectBlock = 1024;

// labels[v] = v, counts = 0
__global__ __launch_bounds__(kBlock) void mc_init_kernel(int V, int* __restrict__ labels, int* __restrict__ counts) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v < V) labels[v] = (int)v;
  if (v < mc::kCountWords) counts[v] = 0;
}

__global__ __launch_bounds__(kBlock) void mc_hook_kernel(int V, int F, const int* __restrict__ faces, int* parent,
                                                          int stamp, int* __restrict__ counts) {
  const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool hooked = false, bad = false;
  if (f < F) {
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    hooked = mc::hook_face(parent, V, a, b, c, &bad);
  }
  const int any_hooked = __syncthreads_or(hooked ? 1 : 0), any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    if (any_hooked) counts[mc::kHookedRound] = stamp;        // once per workgroup; every writer of a round stores the same
    if (any_bad) counts[mc::kStatus] = mc::kStatusBadFace;
  }
}

__global__ __launch_bounds__(kBlock) void mc_compress_kernel(int V, int* parent) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v < V) {
    const int r = mc::find_root(parent, (int)v);
    if (r != (int)v) parent[v] = r;
  }
}

// ---- finish -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mc_clear_kernel(int V, const int* __restrict__ labels, int* __restrict__ fcount,
                                                           int* __restrict__ vcount, unsigned* __restrict__ rank) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  fcount[v] = 0; vcount[v] = 0;
  rank[v] = labels[v] == (int)v ? 1u : 0u;
}

// counter[r] += 1 for every lane with `active`; the lanes that share the first active lane's r add once together
__device__ __forceinline__ void add_one(int* counter, int r, bool active) {
  if (!active) return;
  const int first = __builtin_amdgcn_readfirstlane(r);
  const unsigned long long same = __ballot(r == first);
  if (r != first) atomicAdd(counter + r, 1);
  else if (gs::lane_id() == __ffsll((long long)same) - 1) atomicAdd(counter + first, __popcll(same));
}

__global__ __launch_bounds__(kBlock) void mc_count_kernel(int V, int F, const int* __restrict__ faces,
                                                           const int* __restrict__ labels, int* fcount, int* vcount,
                                                           int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool bad = false;
  int rv = -1, rf = -1;
  if (i < V) {
    rv = labels[i];
    if (!mc::index_ok(rv, V)) { bad = true; rv = -1; }
  }
  if (i < F) {
    const int a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    if (mc::face_ok(a, b, c, V)) {
      rf = labels[a];
      if (!mc::index_ok(rf, V)) { bad = true; rf = -1; }
    }
  }
  add_one(vcount, rv, rv >= 0);
  add_one(fcount, rf, rf >= 0);
  if (__syncthreads_or(bad ? 1 : 0) && threadIdx.x == 0) counts[mc::kStatus] = mc::kStatusBadLabel;
}

// rank: the exclusive scan of the root flags
__global__ __launch_bounds__(kBlock) void mc_table_kernel(int V, const int* __restrict__ labels,
                                                           const unsigned* __restrict__ rank, const int* __restrict__ fcount,
                                                           const int* __restrict__ vcount, int* __restrict__ roots,
                                                           int* __restrict__ tfaces, int* __restrict__ tverts) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V || labels[v] != (int)v) return;
  const unsigned c = rank[v];
  if (c >= (unsigned)V) return;
  roots[c] = (int)v; tfaces[c] = fcount[v]; tverts[c] = vcount[v];
}

__global__ __launch_bounds__(kBlock) void mc_table_copy_kernel(int C, const int* __restrict__ roots,
                                                                const int* __restrict__ tfaces,
                                                                const int* __restrict__ tverts, int* __restrict__ roots_out,
                                                                int* __restrict__ faces_out, int* __restrict__ verts_out) {
  const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  roots_out[c] = roots[c]; faces_out[c] = tfaces[c]; verts_out[c] = tverts[c];
}

// ---- plan ---------------------------------------------------------------------------------------------------------------
// one workgroup: the threshold key of keep_largest (radix select, most significant digit first), keep[root] for every
// component, counts[kKept]
__global__ __launch_bounds__(kSelectBlock) void mc_select_kernel(int V, const int* __restrict__ roots,
                                                                  const int* __restrict__ tfaces, int min_faces,
                                                                  int keep_largest, int* __restrict__ keep,
                                                                  int* __restrict__ counts) {
  __shared__ int hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_k;
  const int t = (int)threadIdx.x;
  int C = counts[mc::kComponents];
  if (C < 0 || C > V) C = 0;
  if (t < 256) hist[t] = 0;
  __syncthreads();
  int mine = 0;
  for (int c = t; c < C; c += kSelectBlock) mine += tfaces[c] >= 1 ? 1 : 0;
  if (mine) atomicAdd(&hist[0], mine);
  __syncthreads();
  const int with_faces = hist[0];
  __syncthreads();
  unsigned long long threshold = 0ull;
  if (keep_largest > 0 && keep_largest < with_faces) {
    if (t == 0) { s_prefix = 0ull; s_k = keep_largest; }
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (int c = t; c < C; c += kSelectBlock) {
        const int fc = tfaces[c];
        if (fc < 1) continue;
        const unsigned long long key = mc::component_key(fc, roots[c]);
        if ((((key ^ prefix) >> shift) >> 8) == 0ull) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (t == 0) {
        int k = s_k, d = 255;
        for (; d > 0; --d) {
          if (hist[d] >= k) break;
          k -= hist[d];
        }
        s_k = k;
        s_prefix = prefix | ((unsigned long long)d << shift);
      }
      __syncthreads();
    }
    threshold = s_prefix;
  }
  __syncthreads();
  if (t == 0) hist[0] = 0;
  __syncthreads();
  int kept = 0;
  for (int c = t; c < C; c += kSelectBlock) {
    const int root = roots[c];
    if (!mc::index_ok(root, V)) continue;
    const int k = mc::survives(tfaces[c], root, threshold, min_faces) ? 1 : 0;
    keep[root] = k;
    kept += k;
  }
  if (kept) atomicAdd(&hist[0], kept);
  __syncthreads();
  if (t == 0) counts[mc::kKept] = hist[0];
}

// the keep flag of vertex v: that of its root; a label outside [0, V) keeps nothing
__device__ __forceinline__ bool vertex_kept(const int* __restrict__ labels, const int* __restrict__ keep, int v, int V) {
  const int r = labels[v];
  return mc::index_ok(r, V) && keep[r] != 0;
}

__global__ __launch_bounds__(kBlock) void mc_flags_kernel(int V, int F, const int* __restrict__ faces,
                                                           const int* __restrict__ labels, const int* __restrict__ keep,
                                                           unsigned* __restrict__ posv, unsigned* __restrict__ posf) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < V) posv[i] = vertex_kept(labels, keep, (int)i, V) ? 1u : 0u;
  if (i < F) {
    const int a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    posf[i] = mc::face_ok(a, b, c, V) && vertex_kept(labels, keep, a, V) ? 1u : 0u;
  }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mc_emit_kernel(int V, int F, const float* __restrict__ verts,
                                                          const int* __restrict__ faces, const float* __restrict__ colors,
                                                          const int* __restrict__ labels, const int* __restrict__ keep,
                                                          const unsigned* __restrict__ posv,
                                                          const unsigned* __restrict__ posf, int V_out, int F_out,
                                                          float* __restrict__ verts_out, int* __restrict__ faces_out,
                                                          float* __restrict__ colors_out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < V && vertex_kept(labels, keep, (int)i, V)) {
    const size_t p = posv[i];
    if (p < (size_t)V_out) {
      for (int q = 0; q < 3; ++q) verts_out[p * 3 + q] = verts[i * 3 + q];
      if (colors_out)
        for (int q = 0; q < 3; ++q) colors_out[p * 3 + q] = colors[i * 3 + q];
    }
  }
  if (i < F) {
    const int a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    if (mc::face_ok(a, b, c, V) && vertex_kept(labels, keep, a, V)) {
      const size_t p = posf[i];
      if (p < (size_t)F_out) {
        faces_out[p * 3] = (int)posv[a]; faces_out[p * 3 + 1] = (int)posv[b]; faces_out[p * 3 + 2] = (int)posv[c];
      }
    }
  }
}

long long align256(long long b) { return (b + 255) & ~255ll; }

struct Layout {
  long long fcount, vcount, rank, roots, tfaces, tverts, keep, posv, posf, scan, scan_bytes, total;
};

Layout layout(int V, int F) {
  Layout L;
  long long o = 0;
  auto take = [&o](long long bytes) { const long long at = o; o += align256(bytes); return at; };
  const long long v4 = 4ll * V;
  L.fcount = take(v4); L.vcount = take(v4); L.rank = take(v4);
  L.roots = take(v4); L.tfaces = take(v4); L.tverts = take(v4);
  L.keep = take(v4); L.posv = take(v4);
  L.posf = take(4ll * F);
  L.scan_bytes = gs_scan_workspace_bytes(V > F ? V : F);
  L.scan = take(L.scan_bytes);
  L.total = o;
  return L;
}

unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

bool sizes_ok(int V, int F) { return V >= 1 && F >= 0; }
bool ws_ok(const void* ws) { return ws && !((uintptr_t)ws & 255); }

#define MC_LAUNCHED() do { const int status_ = gs_launch_status(); if (status_ != GS_OK) return status_; } while (0)
#define MC_CHECK(call) do { const int status_ = (call); if (status_ != GS_OK) return status_; } while (0)

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_mesh_clean_workspace_bytes(int V, int F) {
  if (!sizes_ok(V, F)) return -1;
  return layout(V, F).total;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_components_round(int V, int F, const int* faces, int* labels, int round, int* counts, void* stream) {
  if (!sizes_ok(V, F) || round < 0 || round >= mc::max_rounds(V) || !labels || !counts || (F > 0 && !faces))
    return GS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (round == 0) {
    hipLaunchKernelGGL(mc_init_kernel, dim3(blocks(V > mc::kCountWords ? V : mc::kCountWords)), dim3(kBlock), 0, st, V, labels,
                       counts);
    MC_LAUNCHED();
  }
  if (F == 0) return GS_OK;
  hipLaunchKernelGGL(mc_hook_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, V, F, faces, labels, round + 1, counts);
  MC_LAUNCHED();
  hipLaunchKernelGGL(mc_compress_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, labels);
  MC_LAUNCHED();
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_components_finish(int V, int F, const int* faces, const int* labels, int* counts, void* ws,
                                        long long ws_bytes, void* stream) {
  if (!sizes_ok(V, F) || !labels || !counts || (F > 0 && !faces) || !ws_ok(ws)) return GS_ERR_INVALID;
  const Layout L = layout(V, F);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  char* w = reinterpret_cast<char*>(ws);
  hipStream_t st = (hipStream_t)stream;
  int* fcount = reinterpret_cast<int*>(w + L.fcount);
  int* vcount = reinterpret_cast<int*>(w + L.vcount);
  unsigned* rank = reinterpret_cast<unsigned*>(w + L.rank);
  hipLaunchKernelGGL(mc_clear_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, labels, fcount, vcount, rank);
  MC_LAUNCHED();
  hipLaunchKernelGGL(mc_count_kernel, dim3(blocks(V > F ? V : F)), dim3(kBlock), 0, st, V, F, faces, labels, fcount, vcount,
                     counts);
  MC_LAUNCHED();
  MC_CHECK(gs_exclusive_scan_u32(V, rank, rank, reinterpret_cast<unsigned*>(counts + mc::kComponents), w + L.scan,
                                 L.scan_bytes, stream));
  hipLaunchKernelGGL(mc_table_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, labels, rank, fcount, vcount,
                     reinterpret_cast<int*>(w + L.roots), reinterpret_cast<int*>(w + L.tfaces),
                     reinterpret_cast<int*>(w + L.tverts));
  MC_LAUNCHED();
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_components_table(int V, int F, int C, int* roots, int* face_counts, int* vert_counts, const void* ws,
                                       long long ws_bytes, void* stream) {
  if (!sizes_ok(V, F) || C < 0 || C > V || !ws_ok(ws)) return GS_ERR_INVALID;
  const Layout L = layout(V, F);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  if (C == 0) return GS_OK;
  if (!roots || !face_counts || !vert_counts) return GS_ERR_INVALID;
  const char* w = reinterpret_cast<const char*>(ws);
  hipLaunchKernelGGL(mc_table_copy_kernel, dim3(blocks(C)), dim3(kBlock), 0, (hipStream_t)stream, C,
                     reinterpret_cast<const int*>(w + L.roots), reinterpret_cast<const int*>(w + L.tfaces),
                     reinterpret_cast<const int*>(w + L.tverts), roots, face_counts, vert_counts);
  MC_LAUNCHED();
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_filter_plan(int V, int F, const int* faces, const int* labels, int min_faces, int keep_largest,
                                  int* counts, void* ws, long long ws_bytes, void* stream) {
  if (!sizes_ok(V, F) || F < 1 || min_faces < 0 || keep_largest < 0 || !faces || !labels || !counts || !ws_ok(ws))
    return GS_ERR_INVALID;
  const Layout L = layout(V, F);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  char* w = reinterpret_cast<char*>(ws);
  hipStream_t st = (hipStream_t)stream;
  int* keep = reinterpret_cast<int*>(w + L.keep);
  unsigned* posv = reinterpret_cast<unsigned*>(w + L.posv);
  unsigned* posf = reinterpret_cast<unsigned*>(w + L.posf);
  hipLaunchKernelGGL(mc_select_kernel, dim3(1), dim3(kSelectBlock), 0, st, V, reinterpret_cast<const int*>(w + L.roots),
                     reinterpret_cast<const int*>(w + L.tfaces), min_faces, keep_largest, keep, counts);
  MC_LAUNCHED();
  hipLaunchKernelGGL(mc_flags_kernel, dim3(blocks(V > F ? V : F)), dim3(kBlock), 0, st, V, F, faces, labels, keep, posv, posf);
  MC_LAUNCHED();
  MC_CHECK(gs_exclusive_scan_u32(V, posv, posv, reinterpret_cast<unsigned*>(counts + mc::kVertsOut), w + L.scan,
                                 L.scan_bytes, stream));
  MC_CHECK(gs_exclusive_scan_u32(F, posf, posf, reinterpret_cast<unsigned*>(counts + mc::kFacesOut), w + L.scan,
                                 L.scan_bytes, stream));
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_filter_emit(int V, int F, const float* verts, const int* faces, const float* colors,
                                  const int* labels, int V_out, int F_out, float* verts_out, int* faces_out,
                                  float* colors_out, const void* ws, long long ws_bytes, void* stream) {
  if (!sizes_ok(V, F) || F < 1 || V_out < 0 || F_out < 0 || V_out > V || F_out > F || !verts || !faces || !labels ||
      !ws_ok(ws))
    return GS_ERR_INVALID;
  if ((colors == nullptr) != (colors_out == nullptr)) return GS_ERR_INVALID;
  const Layout L = layout(V, F);
  if (ws_bytes < L.total) return GS_ERR_WORKSPACE;
  if (V_out == 0 && F_out == 0) return GS_OK;
  if (!verts_out || !faces_out) return GS_ERR_INVALID;
  const char* w = reinterpret_cast<const char*>(ws);
  hipLaunchKernelGGL(mc_emit_kernel, dim3(blocks(V > F ? V : F)), dim3(kBlock), 0, (hipStream_t)stream, V, F, verts, faces,
                     colors, labels, reinterpret_cast<const int*>(w + L.keep), reinterpret_cast<const unsigned*>(w + L.posv),
                     reinterpret_cast<const unsigned*>(w + L.posf), V_out, F_out, verts_out, faces_out, colors_out);
  MC_LAUNCHED();
  return GS_OK;
}
