// TEST INFRASTRUCTURE ONLY: csrc/meshclean_math.h compiled for the host (tests/test_meshclean_host.py).  The hook, the root
// walk, the index test, the ranking key and the survivor rule are the kernels'; faces and vertices are visited one after
// the other here, so a hook sees every earlier one of its round.  With -DMESHCLEAN_HOST_MAIN the file is a program of its
// own that runs the small cases (built with -fsanitize=address,undefined by the test).
#include "meshclean_math.h"

#include <algorithm>
#include <functional>
#include <vector>

namespace mc = gs::meshclean;

extern "C" {

int mch_max_rounds(int V) { return mc::max_rounds(V); }
unsigned long long mch_component_key(int face_count, int label) { return mc::component_key(face_count, label); }
int mch_index_ok(int i, int V) { return mc::index_ok(i, V) ? 1 : 0; }

// labels [V]; info[0] = rounds taken, info[1] = status; 0, or 2 when the rounds did not end inside the guard
int mch_components(int V, int F, const int* faces, int* labels, int* info) {
  if (V < 1 || F < 0) return 1;
  for (int v = 0; v < V; ++v) labels[v] = v;
  info[0] = 0; info[1] = 0;
  for (;;) {
    if (info[0] >= mc::max_rounds(V)) return 2;
    ++info[0];
    bool hooked = false, bad = false;
    for (int f = 0; f < F; ++f)
      hooked |= mc::hook_face(labels, V, faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2], &bad);
    if (bad) info[1] = mc::kStatusBadFace;
    for (int v = 0; v < V; ++v) labels[v] = mc::find_root(labels, v);
    if (!hooked) return 0;
  }
}

// count (verts_out == NULL: only counts, as the kernels' words kVertsOut, kFacesOut, kComponents, kKept, kStatus) or emit
int mch_filter(int V, int F, const float* verts, const int* faces, const float* colors, int min_faces, int keep_largest,
               int* counts, float* verts_out, int* faces_out, float* colors_out) {
  if (V < 1 || F < 0 || min_faces < 0 || keep_largest < 0) return 1;
  std::vector<int> labels(V), info(2), fcount(V, 0);
  const int rc = mch_components(V, F, faces, labels.data(), info.data());
  if (rc) return rc;
  counts[mc::kStatus] = info[1];
  for (int f = 0; f < F; ++f) {
    const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    if (mc::face_ok(a, b, c, V)) ++fcount[labels[a]];
  }
  std::vector<unsigned long long> keys;
  int C = 0;
  for (int v = 0; v < V; ++v) {
    if (labels[v] != v) continue;
    ++C;
    if (fcount[v] >= 1) keys.push_back(mc::component_key(fcount[v], v));
  }
  std::sort(keys.begin(), keys.end(), std::greater<unsigned long long>());
  const unsigned long long threshold =
      keep_largest > 0 && (size_t)keep_largest < keys.size() ? keys[(size_t)keep_largest - 1] : 0ull;
  std::vector<int> position(V, -1);
  int V_out = 0, F_out = 0, kept = 0;
  for (int v = 0; v < V; ++v) {
    const int r = labels[v];
    if (!mc::survives(fcount[r], r, threshold, min_faces)) continue;
    kept += r == v ? 1 : 0;
    position[v] = V_out;
    if (verts_out) {
      for (int q = 0; q < 3; ++q) verts_out[(size_t)V_out * 3 + q] = verts[(size_t)v * 3 + q];
      if (colors_out)
        for (int q = 0; q < 3; ++q) colors_out[(size_t)V_out * 3 + q] = colors[(size_t)v * 3 + q];
    }
    ++V_out;
  }
  for (int f = 0; f < F; ++f) {
    const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    if (!mc::face_ok(a, b, c, V) || position[a] < 0) continue;
    if (faces_out) {
      faces_out[(size_t)F_out * 3] = position[a]; faces_out[(size_t)F_out * 3 + 1] = position[b];
      faces_out[(size_t)F_out * 3 + 2] = position[c];
    }
    ++F_out;
  }
  counts[mc::kVertsOut] = V_out; counts[mc::kFacesOut] = F_out; counts[mc::kComponents] = C; counts[mc::kKept] = kept;
  return 0;
}

}  // extern "C"

#ifdef MESHCLEAN_HOST_MAIN
#include <stdio.h>

// the small cases under the sanitizers: a strip of 1025 vertices numbered by a multiplicative scramble, three isolated
// triangles that a duplicate and two degenerate faces bring to 1, 2 and 3 faces, two unreferenced vertices, and two
// faces with an index outside [0, V)
int main() {
  const int S = 1025, V = S + 9 + 2;
  std::vector<int> number(S);
  for (int i = 0; i < S; ++i) number[i] = (int)(((long long)i * 367 + 11) % S);      // 367 and 1025 are coprime
  std::vector<int> faces;
  for (int i = 0; i + 2 < S; ++i) { faces.push_back(number[i]); faces.push_back(number[i + 1]); faces.push_back(number[i + 2]); }
  for (int t = 0; t < 3; ++t) { faces.push_back(S + 3 * t); faces.push_back(S + 3 * t + 1); faces.push_back(S + 3 * t + 2); }
  faces.push_back(S + 3); faces.push_back(S + 4); faces.push_back(S + 5);            // a duplicate: that triangle has 2 faces
  faces.push_back(S + 6); faces.push_back(S + 6); faces.push_back(S + 7);            // degenerate, a == b
  faces.push_back(S + 8); faces.push_back(S + 8); faces.push_back(S + 8);            // degenerate, a == b == c
  const int F_good = (int)faces.size() / 3;
  faces.push_back(-1); faces.push_back(0); faces.push_back(1);
  faces.push_back(0); faces.push_back(1); faces.push_back(V);
  const int F = (int)faces.size() / 3;
  std::vector<float> verts((size_t)V * 3), cols((size_t)V * 3);
  for (int q = 0; q < V * 3; ++q) { verts[q] = 0.5f * (float)q; cols[q] = 1.0f / (float)(q + 1); }
  std::vector<int> labels(V), info(2);
  int rc = mch_components(V, F, faces.data(), labels.data(), info.data());
  int wrong = 0;
  for (int v = 0; v < S; ++v) wrong += labels[v] != 0;
  for (int t = 0; t < 3; ++t)
    for (int q = 0; q < 3; ++q) wrong += labels[S + 3 * t + q] != S + 3 * t;
  wrong += labels[S + 9] != S + 9 || labels[S + 10] != S + 10;
  printf("components: rounds %d of at most %d, status %d, wrong labels %d\n", info[0], mc::max_rounds(V), info[1], wrong);
  rc |= info[1] == mc::kStatusBadFace ? 0 : 4;
  // without the two bad faces: the largest two, then everything with at least 3 faces
  int ok = 1;
  const int want[3][4] = {{1, 0, S, S - 2}, {2, 0, S + 3, S - 2 + 3}, {0, 3, S + 3, S - 2 + 3}};
  for (int n = 0; n < 3; ++n) {
    int counts[mc::kCountWords] = {0};
    rc |= mch_filter(V, F_good, verts.data(), faces.data(), cols.data(), want[n][1], want[n][0], counts, nullptr, nullptr, nullptr);
    std::vector<float> vo((size_t)counts[0] * 3 + 1), co((size_t)counts[0] * 3 + 1);
    std::vector<int> fo((size_t)counts[1] * 3 + 1);
    rc |= mch_filter(V, F_good, verts.data(), faces.data(), cols.data(), want[n][1], want[n][0], counts, vo.data(), fo.data(), co.data());
    for (int q = 0; q < counts[1] * 3; ++q) ok &= fo[q] >= 0 && fo[q] < counts[0];
    ok &= counts[0] == want[n][2] && counts[1] == want[n][3] && counts[mc::kComponents] == 6 && counts[mc::kStatus] == 0;
    printf("filter keep_largest %d min_faces %d: V' %d, F' %d, C %d, kept %d\n", want[n][0], want[n][1], counts[0], counts[1],
           counts[mc::kComponents], counts[mc::kKept]);
  }
  return (rc == 0 && wrong == 0 && ok) ? 0 : 1;
}
#endif
