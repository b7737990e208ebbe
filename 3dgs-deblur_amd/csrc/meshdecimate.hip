// meshdecimate.hip — mesh decimation by vertex clustering with a quadric representative (meshdecimate.py).  The cell, the
// cluster order, the representative and the face rule: meshdecimate_math.h.  gfx950, wave64.  Sorts, scans and float64
// sums in a fixed order: no float atomics (integer atomicAdd only, for two counters), no workgroup waits on another, and
// every word of the workspace is written before it is read, so a run gives the same bits whatever the workspace held.
//
// PLAN   cells        one thread per vertex: the cell (three ints), the x digit as a 32-bit sort key, the status word
//        vertex sort  stable radix sort by x (32 bits), the (z, y) key gathered in that order, stable radix sort by it (64
//                     bits): vertices in ascending (cz, cy, cx, vertex).  The digits are biased cell indices at full
//                     width: the passes do not depend on the data, so plan needs no read-back of its own
//        clusters     head flags, exclusive scan, cluster_of[v] and the first sorted position of every cluster
//        faces        one thread per face: indices tested, cluster triple, degenerate faces counted and dropped
//        dedupe       stable sort of the canonical triples (low id in a 32-bit pass, then (high, mid) in a 64-bit pass);
//                     of a run of equal triples the first — the smallest face index — survives
//        positions    referenced flags per cluster and survivor flags per face, scanned; V', F', C, the two drop counts
//                     and the status wait in counts for one read-back
// EMIT   corners      stable sort of the 3F (cluster, 3 face + corner) pairs, first and last position per cluster
//        solve        one thread per referenced cluster walks its members and its corners in order and solves
//        emit         cluster_of, re-indexed faces
#include "gs_common.h"
#include "meshdecimate_math.h"

namespace {

namespace md = gs::meshdecimate;

constexpr int kBlock = 256;

struct Cell { int x, y, z; };

__device__ __forceinline__ Cell load_cell(const int* __restrict__ cells, size_t v) {
  return Cell{cells[v * 3], cells[v * 3 + 1], cells[v * 3 + 2]};
}

// ---- plan ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void md_cells_kernel(int V, const float* __restrict__ verts, double s,
                                                           int* __restrict__ cells, unsigned* __restrict__ keyx,
                                                           int* __restrict__ counts) {
  const long long v = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool bad = false;
  if (v < V) {
    int c[3];
    for (int k = 0; k < 3; ++k) bad |= !md::cell_of(verts[v * 3 + k], s, &c[k]);
    for (int k = 0; k < 3; ++k) cells[v * 3 + k] = c[k];
    keyx[v] = md::cell_digit(c[0]);
  }
  if (__syncthreads_or(bad ? 1 : 0) && threadIdx.x == 0) counts[md::kStatus] = md::kStatusBadVertex;
}

// order: the vertices sorted by x.  key[i] = the (z, y) key of order[i]
__global__ __launch_bounds__(kBlock) void md_key_zy_kernel(int V, const unsigned* __restrict__ order,
                                                            const int* __restrict__ cells,
                                                            unsigned long long* __restrict__ key) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  const unsigned v = order[i];
  if (v >= (unsigned)V) { key[i] = 0ull; return; }
  key[i] = md::cell_key_zy(cells[(size_t)v * 3 + 1], cells[(size_t)v * 3 + 2]);
}

// order: the vertices in cluster order.  perm = order, head[i] = 1 where a cluster begins; ref = 0
__global__ __launch_bounds__(kBlock) void md_heads_kernel(int V, const unsigned* __restrict__ order,
                                                           const int* __restrict__ cells, int* __restrict__ perm,
                                                           unsigned* __restrict__ head, unsigned* __restrict__ ref) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  unsigned v = order[i];
  if (v >= (unsigned)V) v = 0u;
  perm[i] = (int)v;
  ref[i] = 0u;
  unsigned h = 1u;
  if (i > 0) {
    unsigned u = order[i - 1];
    if (u >= (unsigned)V) u = 0u;
    const Cell a = load_cell(cells, v), b = load_cell(cells, u);
    h = (a.x != b.x || a.y != b.y || a.z != b.z) ? 1u : 0u;
  }
  head[i] = h;
}

// before: the exclusive scan of head.  cluster_of[perm[i]], cstart[cluster] = its first sorted position
__global__ __launch_bounds__(kBlock) void md_assign_kernel(int V, const int* __restrict__ perm,
                                                            const unsigned* __restrict__ head,
                                                            const unsigned* __restrict__ before,
                                                            int* __restrict__ cluster_of, int* __restrict__ cstart) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  const unsigned h = head[i];
  const unsigned id = before[i] + h - 1u;
  if (id >= (unsigned)V) return;
  cluster_of[perm[i]] = (int)id;
  if (h) cstart[id] = (int)i;
}

// the clusters of a face's corners -> false (and nothing read through a bad index) when an index is outside [0, V)
__device__ __forceinline__ bool face_clusters(const int* __restrict__ faces, const int* __restrict__ cluster_of, int V,
                                              size_t f, int* a, int* b, int* c) {
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  if (!md::face_ok(ia, ib, ic, V)) return false;
  *a = cluster_of[ia]; *b = cluster_of[ib]; *c = cluster_of[ic];
  return md::face_ok(*a, *b, *c, V);
}

__device__ __forceinline__ void mark(unsigned* __restrict__ ref, int a, int b, int c) {
  ref[a] = 1u; ref[b] = 1u; ref[c] = 1u;          // every writer stores the same word
}

__global__ __launch_bounds__(kBlock) void md_faces_kernel(int V, int F, const int* __restrict__ faces,
                                                           const int* __restrict__ cluster_of, int dedupe,
                                                           int* __restrict__ tri, unsigned* __restrict__ surv,
                                                           unsigned* __restrict__ keylo, unsigned* __restrict__ ref,
                                                           int* __restrict__ counts) {
  const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool bad = false, degenerate = false;
  if (f < F) {
    int a = 0, b = 0, c = 0, lo = 0, mid = 0, hi = 0;
    unsigned alive = 0u;
    if (!face_clusters(faces, cluster_of, V, (size_t)f, &a, &b, &c)) {
      bad = true;
    } else if (md::degenerate(a, b, c)) {
      degenerate = true;
      md::sort3(a, b, c, &lo, &mid, &hi);
    } else {
      alive = 1u;
      md::sort3(a, b, c, &lo, &mid, &hi);
      if (!dedupe) mark(ref, a, b, c);
    }
    surv[f] = alive;
    if (dedupe) {
      tri[f * 3] = lo; tri[f * 3 + 1] = mid; tri[f * 3 + 2] = hi;
      keylo[f] = (unsigned)lo;
    }
  }
  const int n_deg = __syncthreads_count(degenerate ? 1 : 0);
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x == 0) {
    if (n_deg) atomicAdd(counts + md::kDegenerate, n_deg);
    if (any_bad) counts[md::kStatus] = md::kStatusBadFace;
  }
}

// order: the faces sorted by their low id.  key[i] = (hi << bits) | mid of order[i]
__global__ __launch_bounds__(kBlock) void md_key_himid_kernel(int F, const unsigned* __restrict__ order,
                                                               const int* __restrict__ tri, int bits,
                                                               unsigned long long* __restrict__ key) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= F) return;
  const unsigned f = order[i];
  if (f >= (unsigned)F) { key[i] = 0ull; return; }
  key[i] = ((unsigned long long)(unsigned)tri[(size_t)f * 3 + 2] << bits) | (unsigned long long)(unsigned)tri[(size_t)f * 3 + 1];
}

// order: the faces sorted by canonical triple, equal triples in ascending face index
__global__ __launch_bounds__(kBlock) void md_dedupe_kernel(int V, int F, const unsigned* __restrict__ order,
                                                            const int* __restrict__ faces,
                                                            const int* __restrict__ cluster_of,
                                                            const int* __restrict__ tri, unsigned* __restrict__ surv,
                                                            unsigned* __restrict__ ref, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool duplicate = false;
  if (i < F) {
    const unsigned f = order[i];
    if (f < (unsigned)F && surv[f]) {
      if (i > 0) {
        const unsigned g = order[i - 1];
        if (g < (unsigned)F)
          duplicate = tri[(size_t)f * 3] == tri[(size_t)g * 3] && tri[(size_t)f * 3 + 1] == tri[(size_t)g * 3 + 1] &&
                      tri[(size_t)f * 3 + 2] == tri[(size_t)g * 3 + 2];
      }
      int a, b, c;
      if (duplicate) surv[f] = 0u;
      else if (face_clusters(faces, cluster_of, V, (size_t)f, &a, &b, &c)) mark(ref, a, b, c);
    }
  }
  const int n_dup = __syncthreads_count(duplicate ? 1 : 0);
  if (threadIdx.x == 0 && n_dup) atomicAdd(counts + md::kDuplicates, n_dup);
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void md_corners_kernel(int V, int F, const int* __restrict__ faces,
                                                             const int* __restrict__ cluster_of,
                                                             unsigned* __restrict__ key, int* __restrict__ fbeg,
                                                             int* __restrict__ fend) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < V) { fbeg[i] = 0; fend[i] = 0; }
  if (i >= 3ll * F) return;
  const size_t f = (size_t)(i / 3);
  const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
  unsigned k = 0u;
  if (md::face_ok(ia, ib, ic, V)) {
    const int c = cluster_of[faces[i]];
    if (md::index_ok(c, V)) k = (unsigned)c;
  }
  key[i] = k;
}

__global__ __launch_bounds__(kBlock) void md_bounds_kernel(int V, long long n, const unsigned* __restrict__ key,
                                                            int* __restrict__ fbeg, int* __restrict__ fend) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned k = key[i];
  if (k >= (unsigned)V) return;
  if (i == 0 || key[i - 1] != k) fbeg[k] = (int)i;
  if (i == n - 1 || key[i + 1] != k) fend[k] = (int)(i + 1);
}

__global__ __launch_bounds__(kBlock) void md_solve_kernel(int V, int F, const float* __restrict__ verts,
                                                           const int* __restrict__ faces,
                                                           const float* __restrict__ colors, double s,
                                                           const int* __restrict__ counts, const int* __restrict__ cells,
                                                           const int* __restrict__ perm, const int* __restrict__ cstart,
                                                           const unsigned* __restrict__ ref,
                                                           const unsigned* __restrict__ posv,
                                                           const int* __restrict__ fbeg, const int* __restrict__ fend,
                                                           const unsigned* __restrict__ corner, int V_out,
                                                           float* __restrict__ verts_out, float* __restrict__ colors_out) {
  const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
  int C = counts[md::kClusters];
  if (C < 0 || C > V) C = 0;
  if (c >= C || !ref[c]) return;
  const size_t p = posv[c];
  if (p >= (size_t)V_out) return;
  int begin = cstart[c], end = c + 1 < C ? cstart[c + 1] : V;
  if (begin < 0 || begin >= V || end <= begin || end > V) return;
  md::Cluster q;
  const Cell cell = load_cell(cells, (size_t)perm[begin]);
  md::cluster_begin(&q, cell.x, cell.y, cell.z, s);
  for (int i = begin; i < end; ++i) {
    const size_t v = (size_t)perm[i];
    md::cluster_add_member(&q, verts + v * 3, colors_out ? colors + v * 3 : nullptr);
  }
  long long j0 = fbeg[c], j1 = fend[c];
  if (j0 < 0 || j1 > 3ll * F || j1 < j0) j1 = j0 = 0;
  for (long long j = j0; j < j1; ++j) {
    const size_t f = (size_t)(corner[j] / 3u);
    if (f >= (size_t)F) continue;
    const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (!md::face_ok(ia, ib, ic, V)) continue;
    md::cluster_add_face(&q, verts + (size_t)ia * 3, verts + (size_t)ib * 3, verts + (size_t)ic * 3);
  }
  float out[3], col[3];
  md::cluster_solve(&q, s, out, colors_out ? col : nullptr);
  for (int k = 0; k < 3; ++k) verts_out[p * 3 + k] = out[k];
  if (colors_out)
    for (int k = 0; k < 3; ++k) colors_out[p * 3 + k] = col[k];
}

__global__ __launch_bounds__(kBlock) void md_emit_kernel(int V, int F, const int* __restrict__ faces,
                                                          const int* __restrict__ cluster_of,
                                                          const unsigned* __restrict__ ref,
                                                          const unsigned* __restrict__ posv,
                                                          const unsigned* __restrict__ surv,
                                                          const unsigned* __restrict__ posf, int V_out, int F_out,
                                                          int* __restrict__ faces_out, int* __restrict__ map_out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (map_out && i < V) {
    const int c = cluster_of[i];
    map_out[i] = md::index_ok(c, V) && ref[c] && posv[c] < (unsigned)V_out ? (int)posv[c] : -1;
  }
  if (faces_out && i < F && surv[i]) {
    const size_t p = posf[i];
    int a, b, c;
    if (p < (size_t)F_out && face_clusters(faces, cluster_of, V, (size_t)i, &a, &b, &c)) {
      faces_out[p * 3] = (int)posv[a]; faces_out[p * 3 + 1] = (int)posv[b]; faces_out[p * 3 + 2] = (int)posv[c];
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
long long align256(long long b) { return (b + 255) & ~255ll; }
long long max2(long long a, long long b) { return a > b ? a : b; }

struct Layout {
  long long cells, perm, head, before, cluster_of, cstart, ref, posv, fbeg, fend, tri, surv, posf;
  long long k32[2], val[2], k64[2];      // the sort buffers: vertices and faces in plan, 3F corners (k32, val) in emit
  long long scan, scan_bytes, sort, sort_bytes, total;
  int bits;
};

Layout layout(int V, int F) {
  Layout L;
  long long o = 0;
  auto take = [&o](long long bytes) { const long long at = o; o += align256(bytes); return at; };
  const long long v4 = 4ll * V, f4 = 4ll * F;
  L.cells = take(3 * v4); L.perm = take(v4); L.head = take(v4); L.before = take(v4); L.cluster_of = take(v4);
  L.cstart = take(v4); L.ref = take(v4); L.posv = take(v4); L.fbeg = take(v4); L.fend = take(v4);
  L.tri = take(3 * f4); L.surv = take(f4); L.posf = take(f4);
  const long long n32 = max2(V, 3ll * F), n64 = max2(V, F);
  for (int q = 0; q < 2; ++q) L.k32[q] = take(4 * n32);
  for (int q = 0; q < 2; ++q) L.val[q] = take(4 * n32);
  for (int q = 0; q < 2; ++q) L.k64[q] = take(8 * n64);
  L.bits = md::index_bits(V);
  L.scan_bytes = gs_scan_workspace_bytes(max2(V, F));
  L.scan = take(L.scan_bytes);
  // one query per sort that plan and emit issue
  L.sort_bytes = max2(gs_radix_sort_workspace_bytes(V, 0, 32), gs_radix_sort_workspace_bytes(V, 0, 64));
  L.sort_bytes = max2(L.sort_bytes, gs_radix_sort_workspace_bytes(F, 0, L.bits));
  L.sort_bytes = max2(L.sort_bytes, gs_radix_sort_workspace_bytes(F, 0, 2 * L.bits));
  L.sort_bytes = max2(L.sort_bytes, gs_radix_sort_workspace_bytes(3ll * F, 0, L.bits));
  L.sort = take(L.sort_bytes);
  L.total = o;
  return L;
}

unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

bool sizes_ok(int V, int F) { return V >= 1 && F >= 1 && V <= md::kMaxVerts && F <= md::kMaxFaces; }

bool desc_ok(const gs_mesh_decimate_desc* d) {
  return d && sizes_ok(d->V, d->F) && d->verts && d->faces && d->counts && d->ws && !((uintptr_t)d->ws & 255) &&
         d->cell_size > 0.0 && d->cell_size - d->cell_size == 0.0;
}

#define MD_LAUNCHED() do { const int status_ = gs_launch_status(); if (status_ != GS_OK) return status_; } while (0)
#define MD_CHECK(call) do { const int status_ = (call); if (status_ != GS_OK) return status_; } while (0)

template <typename T>
T* at(void* ws, long long offset) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + offset); }

}  // namespace

// see include/gsdeblur.h
GS_EXPORT long long gs_mesh_decimate_workspace_bytes(int V, int F) {
  if (!sizes_ok(V, F)) return -1;
  return layout(V, F).total;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_decimate_plan(const gs_mesh_decimate_desc* d) {
  if (!desc_ok(d)) return GS_ERR_INVALID;
  const int V = d->V, F = d->F;
  const Layout L = layout(V, F);
  if (d->ws_bytes < L.total) return GS_ERR_WORKSPACE;
  void* w = d->ws;
  hipStream_t st = (hipStream_t)d->stream;
  int* cells = at<int>(w, L.cells);
  int* perm = at<int>(w, L.perm);
  unsigned* head = at<unsigned>(w, L.head);
  unsigned* before = at<unsigned>(w, L.before);
  int* cluster_of = at<int>(w, L.cluster_of);
  unsigned* ref = at<unsigned>(w, L.ref);
  unsigned* surv = at<unsigned>(w, L.surv);
  int* tri = at<int>(w, L.tri);
  unsigned* k32[2] = {at<unsigned>(w, L.k32[0]), at<unsigned>(w, L.k32[1])};
  unsigned* val[2] = {at<unsigned>(w, L.val[0]), at<unsigned>(w, L.val[1])};
  unsigned long long* k64[2] = {at<unsigned long long>(w, L.k64[0]), at<unsigned long long>(w, L.k64[1])};
  void* sort_ws = at<char>(w, L.sort);
  void* scan_ws = at<char>(w, L.scan);

  const hipError_t e = hipMemsetAsync(d->counts, 0, sizeof(int) * md::kCountWords, st);
  if (e != hipSuccess) return 1000 + (int)e;
  hipLaunchKernelGGL(md_cells_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, d->verts, d->cell_size, cells, k32[0],
                     d->counts);
  MD_LAUNCHED();
  int r = 0;
  MD_CHECK(gs_radix_sort_pairs_u32(V, k32[0], val[0], k32[1], val[1], 1, 0, 32, sort_ws, L.sort_bytes, &r, d->stream));
  hipLaunchKernelGGL(md_key_zy_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, val[r], cells, k64[0]);
  MD_LAUNCHED();
  int r2 = 0;
  MD_CHECK(gs_radix_sort_pairs_u64(V, k64[0], val[r], k64[1], val[r ^ 1], 0, 0, 64, sort_ws, L.sort_bytes, &r2, d->stream));
  const unsigned* order = r2 == 0 ? val[r] : val[r ^ 1];
  hipLaunchKernelGGL(md_heads_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, order, cells, perm, head, ref);
  MD_LAUNCHED();
  MD_CHECK(gs_exclusive_scan_u32(V, head, before, reinterpret_cast<unsigned*>(d->counts + md::kClusters), scan_ws,
                                 L.scan_bytes, d->stream));
  hipLaunchKernelGGL(md_assign_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, perm, head, before, cluster_of,
                     at<int>(w, L.cstart));
  MD_LAUNCHED();
  hipLaunchKernelGGL(md_faces_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, V, F, d->faces, cluster_of, d->dedupe ? 1 : 0,
                     tri, surv, k32[0], ref, d->counts);
  MD_LAUNCHED();
  if (d->dedupe) {
    MD_CHECK(gs_radix_sort_pairs_u32(F, k32[0], val[0], k32[1], val[1], 1, 0, L.bits, sort_ws, L.sort_bytes, &r, d->stream));
    hipLaunchKernelGGL(md_key_himid_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, F, val[r], tri, L.bits, k64[0]);
    MD_LAUNCHED();
    MD_CHECK(gs_radix_sort_pairs_u64(F, k64[0], val[r], k64[1], val[r ^ 1], 0, 0, 2 * L.bits, sort_ws, L.sort_bytes, &r2,
                                     d->stream));
    hipLaunchKernelGGL(md_dedupe_kernel, dim3(blocks(F)), dim3(kBlock), 0, st, V, F, r2 == 0 ? val[r] : val[r ^ 1], d->faces,
                       cluster_of, tri, surv, ref, d->counts);
    MD_LAUNCHED();
  }
  MD_CHECK(gs_exclusive_scan_u32(V, ref, at<unsigned>(w, L.posv), reinterpret_cast<unsigned*>(d->counts + md::kVertsOut),
                                 scan_ws, L.scan_bytes, d->stream));
  MD_CHECK(gs_exclusive_scan_u32(F, surv, at<unsigned>(w, L.posf), reinterpret_cast<unsigned*>(d->counts + md::kFacesOut),
                                 scan_ws, L.scan_bytes, d->stream));
  return GS_OK;
}

// see include/gsdeblur.h
GS_EXPORT int gs_mesh_decimate_emit(const gs_mesh_decimate_desc* d) {
  if (!desc_ok(d)) return GS_ERR_INVALID;
  const int V = d->V, F = d->F;
  if (d->V_out < 0 || d->F_out < 0 || d->V_out > V || d->F_out > F) return GS_ERR_INVALID;
  if (d->colors_out && !d->colors) return GS_ERR_INVALID;
  if ((d->V_out > 0 && !d->verts_out) || (d->F_out > 0 && !d->faces_out)) return GS_ERR_INVALID;
  const Layout L = layout(V, F);
  if (d->ws_bytes < L.total) return GS_ERR_WORKSPACE;
  void* w = d->ws;
  hipStream_t st = (hipStream_t)d->stream;
  const int* cluster_of = at<int>(w, L.cluster_of);
  const unsigned* ref = at<unsigned>(w, L.ref);
  const unsigned* posv = at<unsigned>(w, L.posv);
  if (d->V_out > 0) {
    unsigned* k32[2] = {at<unsigned>(w, L.k32[0]), at<unsigned>(w, L.k32[1])};
    unsigned* val[2] = {at<unsigned>(w, L.val[0]), at<unsigned>(w, L.val[1])};
    int* fbeg = at<int>(w, L.fbeg);
    int* fend = at<int>(w, L.fend);
    const long long n = 3ll * F;
    hipLaunchKernelGGL(md_corners_kernel, dim3(blocks(n > V ? n : V)), dim3(kBlock), 0, st, V, F, d->faces, cluster_of,
                       k32[0], fbeg, fend);
    MD_LAUNCHED();
    int r = 0;
    MD_CHECK(gs_radix_sort_pairs_u32(n, k32[0], val[0], k32[1], val[1], 1, 0, L.bits, at<char>(w, L.sort), L.sort_bytes, &r,
                                     d->stream));
    hipLaunchKernelGGL(md_bounds_kernel, dim3(blocks(n)), dim3(kBlock), 0, st, V, n, k32[r], fbeg, fend);
    MD_LAUNCHED();
    hipLaunchKernelGGL(md_solve_kernel, dim3(blocks(V)), dim3(kBlock), 0, st, V, F, d->verts, d->faces, d->colors,
                       d->cell_size, d->counts, at<int>(w, L.cells), at<int>(w, L.perm), at<int>(w, L.cstart), ref, posv, fbeg,
                       fend, val[r], d->V_out, d->verts_out, d->colors_out);
    MD_LAUNCHED();
  }
  if (d->cluster_of || d->F_out > 0) {
    hipLaunchKernelGGL(md_emit_kernel, dim3(blocks(V > F ? V : F)), dim3(kBlock), 0, st, V, F, d->faces, cluster_of, ref, posv,
                       at<unsigned>(w, L.surv), at<unsigned>(w, L.posf), d->V_out, d->F_out,
                       d->F_out > 0 ? d->faces_out : nullptr, d->cluster_of);
    MD_LAUNCHED();
  }
  return GS_OK;
}
