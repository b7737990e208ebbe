// meshclean_math.h — connected components of a triangle mesh and the removal of small ones (meshclean.py).  Shared by
// csrc/meshclean.hip and the host build of tests/host_math/meshclean_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement
// as tsdf_math.h).  Integers only.
//
// GRAPH    the V vertices are the nodes, the three sides of every face the edges.  labels[v] is the smallest vertex index
//          of v's component: a pure function of the mesh.  A vertex no face refers to is a component with 0 faces; a face
//          belongs to the component of its vertices (its own sides connect them, degenerate faces included).
// ROUNDS   parent [V], parent[v] = v at the start, parent[v] <= v always.
//   hook      for every side (a, b) of every face: ra = root(a), rb = root(b) (follow parent until parent[r] == r); if they
//             differ, parent[max(ra, rb)] = min(parent[max(ra, rb)], min(ra, rb)) and the round "hooked"
//   compress  parent[v] = root(v) for every vertex
//   A round that hooked nothing ends the loop: parent is then the labels.  root() only ever walks to smaller indices, so it
//   ends in at most V steps whatever it reads; a value read late is an older ancestor of the same component, so a hook
//   never joins two components and can at worst be redundant.  A face with an index outside [0, V) is skipped and
//   recorded (kStatusBadFace); no such index is ever used as an address.
// FILTER   rank the components that have at least one face by (face count descending, label ascending): by the key
//          (face_count << 32) | (0x7fffffff - label), descending.  keep_largest = K > 0: only the first min(K, C) of that
//          ranking survive (strict: ties go to the smaller label); K = 0: all of them.  Of the survivors those with fewer
//          than min_faces faces are dropped; components with 0 faces are always dropped.  Surviving vertices and faces
//          keep their relative order; faces are re-indexed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_MC_HD __host__ __device__ __forceinline__
#else
#define GS_MC_HD inline
#endif

namespace gs {
namespace meshclean {

// the words of `counts` (device, kCountWords ints) that the entries fill and the caller reads back once
constexpr int kCountWords = 8;
constexpr int kVertsOut = 0, kFacesOut = 1, kComponents = 2, kKept = 3, kStatus = 4, kHookedRound = 5;
constexpr int kStatusBadFace = 1;      // a face index outside [0, V)
constexpr int kStatusBadLabel = 2;     // a label outside [0, V): the rounds were not run on this buffer

GS_MC_HD bool index_ok(int i, int V) { return (unsigned)i < (unsigned)V; }
GS_MC_HD bool face_ok(int a, int b, int c, int V) { return index_ok(a, V) && index_ok(b, V) && index_ok(c, V); }

// the rounds a correct run stays far inside (a condition that shows a defect, not a tuning number)
GS_MC_HD int bit_length(int v) {
  int n = 0;
  while (v > 0) { ++n; v >>= 1; }
  return n;
}
GS_MC_HD int max_rounds(int V) { return 8 * bit_length(V) + 8; }

GS_MC_HD int find_root(const int* parent, int v) {
  for (;;) {
    const int p = parent[v];
    if ((unsigned)p >= (unsigned)v) return v;      // p == v: a root (anything else outside [0, v) never occurs; it ends the
    v = p;                                         // walk too, so the walk stays inside the array on any buffer)
  }
}

// parent[at] = min(parent[at], value); on the device an integer atomic, so the result does not depend on the order
GS_MC_HD void store_min(int* parent, int at, int value) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(parent + at, value);
#else
  if (value < parent[at]) parent[at] = value;
#endif
}

// one side of a face; a and b are valid indices.  true: the roots differed and one was hooked under the other
GS_MC_HD bool hook_side(int* parent, int a, int b) {
  const int ra = find_root(parent, a), rb = find_root(parent, b);
  if (ra == rb) return false;
  store_min(parent, ra > rb ? ra : rb, ra > rb ? rb : ra);
  return true;
}

// the three sides of one face -> hooked; *bad is set for a face with an index outside [0, V), which is skipped whole
GS_MC_HD bool hook_face(int* parent, int V, int a, int b, int c, bool* bad) {
  if (!face_ok(a, b, c, V)) { *bad = true; return false; }
  bool hooked = hook_side(parent, a, b);
  hooked |= hook_side(parent, b, c);
  hooked |= hook_side(parent, c, a);
  return hooked;
}

// the ranking key of a component with face_count >= 1: larger is better
GS_MC_HD unsigned long long component_key(int face_count, int label) {
  return ((unsigned long long)(unsigned)face_count << 32) | (unsigned long long)(0x7fffffff - label);
}

// threshold: the key of the last component that keep_largest lets through (0: no limit)
GS_MC_HD bool survives(int face_count, int label, unsigned long long threshold, int min_faces) {
  return face_count >= 1 && face_count >= min_faces && component_key(face_count, label) >= threshold;
}

}  // namespace meshclean
}  // namespace gs
