// TEST INFRASTRUCTURE ONLY: csrc/meshdecimate_math.h compiled for the host (tests/test_meshdecimate_host.py).  The cell, the
// sums of a cluster, the solve, the canonical triple and the index tests are the kernels'; the sorting and the compaction
// around them are std::sort and plain loops.  Compile with -ffp-contract=off, as the kernels are.  With
// -DMESHDECIMATE_HOST_MAIN the file is a program of its own that runs the small cases (built with
// -fsanitize=address,undefined by the test).
#include "meshdecimate_math.h"

#include <algorithm>
#include <array>
#include <limits>
#include <map>
#include <vector>

namespace md = gs::meshdecimate;

extern "C" {

int mdh_cell_of(float v, double s, int* c) { return md::cell_of(v, s, c) ? 1 : 0; }
int mdh_index_bits(int n) { return md::index_bits(n); }

// count (verts_out == NULL: only counts, as the kernels' words) or emit.  0, or 1 on arguments outside the limits
int mdh_decimate(int V, int F, const float* verts, const int* faces, const float* colors, double s, int dedupe, int* counts,
                 float* verts_out, int* faces_out, float* colors_out, int* cluster_of_out) {
  if (V < 1 || F < 1 || !(s > 0.0)) return 1;
  for (int k = 0; k < md::kCountWords; ++k) counts[k] = 0;
  std::vector<std::array<int, 3>> cells(V);
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k)
      if (!md::cell_of(verts[(size_t)v * 3 + k], s, &cells[v][k])) counts[md::kStatus] = md::kStatusBadVertex;
  for (int f = 0; f < F; ++f)
    if (!md::face_ok(faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2], V))
      counts[md::kStatus] = md::kStatusBadFace;
  if (counts[md::kStatus]) return 0;
  // clusters: vertices in ascending (cz, cy, cx, vertex)
  std::vector<int> perm(V);
  for (int v = 0; v < V; ++v) perm[v] = v;
  auto key = [&](int v) { return std::array<unsigned long long, 2>{md::cell_key_zy(cells[v][1], cells[v][2]), md::cell_digit(cells[v][0])}; };
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return key(a) < key(b); });
  std::vector<int> cluster_of(V), cstart;
  for (int i = 0; i < V; ++i) {
    if (i == 0 || cells[perm[i]] != cells[perm[i - 1]]) cstart.push_back(i);
    cluster_of[perm[i]] = (int)cstart.size() - 1;
  }
  const int C = (int)cstart.size();
  cstart.push_back(V);
  // faces
  std::vector<char> surv(F, 0), ref(C, 0);
  std::map<std::array<int, 3>, int> first;
  for (int f = 0; f < F; ++f) {
    const int a = cluster_of[faces[(size_t)f * 3]], b = cluster_of[faces[(size_t)f * 3 + 1]], c = cluster_of[faces[(size_t)f * 3 + 2]];
    if (md::degenerate(a, b, c)) { ++counts[md::kDegenerate]; continue; }
    if (dedupe) {
      std::array<int, 3> t;
      md::sort3(a, b, c, &t[0], &t[1], &t[2]);
      if (!first.emplace(t, f).second) { ++counts[md::kDuplicates]; continue; }
    }
    surv[f] = 1; ref[a] = ref[b] = ref[c] = 1;
  }
  std::vector<int> posv(C, -1);
  int V_out = 0, F_out = 0;
  for (int c = 0; c < C; ++c)
    if (ref[c]) posv[c] = V_out++;
  for (int f = 0; f < F; ++f) F_out += surv[f];
  counts[md::kVertsOut] = V_out; counts[md::kFacesOut] = F_out; counts[md::kClusters] = C;
  if (!verts_out) return 0;
  // corners per cluster in ascending (face, corner)
  std::vector<std::vector<int>> corners(C);
  for (int f = 0; f < F; ++f)
    for (int k = 0; k < 3; ++k) corners[cluster_of[faces[(size_t)f * 3 + k]]].push_back(f);
  for (int c = 0; c < C; ++c) {
    if (!ref[c]) continue;
    md::Cluster q;
    const std::array<int, 3>& cell = cells[perm[cstart[c]]];
    md::cluster_begin(&q, cell[0], cell[1], cell[2], s);
    for (int i = cstart[c]; i < cstart[c + 1]; ++i)
      md::cluster_add_member(&q, verts + (size_t)perm[i] * 3, colors_out ? colors + (size_t)perm[i] * 3 : nullptr);
    for (int f : corners[c])
      md::cluster_add_face(&q, verts + (size_t)faces[(size_t)f * 3] * 3, verts + (size_t)faces[(size_t)f * 3 + 1] * 3,
                           verts + (size_t)faces[(size_t)f * 3 + 2] * 3);
    md::cluster_solve(&q, s, verts_out + (size_t)posv[c] * 3, colors_out ? colors_out + (size_t)posv[c] * 3 : nullptr);
  }
  int at = 0;
  for (int f = 0; f < F; ++f) {
    if (!surv[f]) continue;
    for (int k = 0; k < 3; ++k) faces_out[(size_t)at * 3 + k] = posv[cluster_of[faces[(size_t)f * 3 + k]]];
    ++at;
  }
  if (cluster_of_out)
    for (int v = 0; v < V; ++v) cluster_of_out[v] = posv[cluster_of[v]];
  return 0;
}

}  // extern "C"

#ifdef MESHDECIMATE_HOST_MAIN
#include <stdio.h>

// the small cases under the sanitizers: the unit cube as a soup of 12 triangles welded at s = 1/8 (8 vertices at the
// corners, where three planes meet), a tetrahedron inside one cell (everything collapses), a pseudo-random soup of 1025
// vertices and 1023 faces with repeated faces, and the three refusals
int main() {
  int rc = 0;
  int counts[md::kCountWords];
  {
    const int q[6][4][3] = {{{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 0}}, {{0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}},
                            {{0, 0, 0}, {1, 0, 0}, {1, 0, 1}, {0, 0, 1}}, {{0, 1, 0}, {0, 1, 1}, {1, 1, 1}, {1, 1, 0}},
                            {{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {0, 1, 0}}, {{1, 0, 0}, {1, 1, 0}, {1, 1, 1}, {1, 0, 1}}};
    std::vector<float> verts;
    std::vector<int> faces;
    const int order[6] = {0, 1, 2, 0, 2, 3};
    for (int s = 0; s < 6; ++s)
      for (int k = 0; k < 6; ++k)
        for (int a = 0; a < 3; ++a) verts.push_back((float)q[s][order[k]][a]);
    for (int i = 0; i < 36; ++i) faces.push_back(i);
    rc |= mdh_decimate(36, 12, verts.data(), faces.data(), nullptr, 0.125, 1, counts, nullptr, nullptr, nullptr, nullptr);
    std::vector<float> vo((size_t)counts[0] * 3 + 1);
    std::vector<int> fo((size_t)counts[1] * 3 + 1), map(36);
    rc |= mdh_decimate(36, 12, verts.data(), faces.data(), nullptr, 0.125, 1, counts, vo.data(), fo.data(), nullptr, map.data());
    double worst = 0.0;
    for (int i = 0; i < 36; ++i)
      for (int a = 0; a < 3; ++a) {
        const double e = (double)vo[(size_t)map[i] * 3 + a] - (double)verts[(size_t)i * 3 + a];
        worst = std::max(worst, e < 0 ? -e : e);
      }
    printf("cube: V' %d, F' %d, C %d, corner error %.3g\n", counts[0], counts[1], counts[2], worst);
    rc |= (counts[0] == 8 && counts[1] == 12 && worst < 1e-6) ? 0 : 2;
  }
  {
    const float verts[12] = {0.1f, 0.1f, 0.1f, 0.4f, 0.1f, 0.1f, 0.1f, 0.4f, 0.1f, 0.1f, 0.1f, 0.4f};
    const int faces[12] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
    rc |= mdh_decimate(4, 4, verts, faces, nullptr, 1.0, 1, counts, nullptr, nullptr, nullptr, nullptr);
    printf("tetrahedron: V' %d, F' %d, degenerate %d\n", counts[0], counts[1], counts[md::kDegenerate]);
    rc |= (counts[0] == 0 && counts[1] == 0 && counts[md::kDegenerate] == 4) ? 0 : 4;
  }
  {
    const int V = 1025, F = 1023;
    std::vector<float> verts((size_t)V * 3), cols((size_t)V * 3);
    std::vector<int> faces((size_t)F * 3);
    unsigned long long x = 88172645463325252ull;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (size_t i = 0; i < verts.size(); ++i) {
      verts[i] = (float)((double)(next() % 12001) / 2000.0 - 3.0);
      if (next() % 5 == 0) verts[i] = 0.5f * (float)((int)(next() % 13) - 6);
      cols[i] = (float)(next() % 1000) / 999.0f;
    }
    for (size_t i = 0; i < faces.size(); ++i) faces[i] = (int)(next() % V);
    for (int f = 8; f < F; f += 8)
      for (int k = 0; k < 3; ++k) faces[(size_t)f * 3 + k] = faces[(size_t)(f - 5) * 3 + 2 - k];
    for (int dedupe = 0; dedupe < 2; ++dedupe) {
      rc |= mdh_decimate(V, F, verts.data(), faces.data(), cols.data(), 0.5, dedupe, counts, nullptr, nullptr, nullptr, nullptr);
      std::vector<float> vo((size_t)counts[0] * 3 + 1), co((size_t)counts[0] * 3 + 1);
      std::vector<int> fo((size_t)counts[1] * 3 + 1), map(V);
      rc |= mdh_decimate(V, F, verts.data(), faces.data(), cols.data(), 0.5, dedupe, counts, vo.data(), fo.data(), co.data(), map.data());
      int ok = 1;
      for (int i = 0; i < counts[1] * 3; ++i) ok &= fo[i] >= 0 && fo[i] < counts[0];
      for (int v = 0; v < V; ++v) ok &= map[v] >= -1 && map[v] < counts[0];
      printf("soup dedupe %d: V' %d, F' %d, C %d, degenerate %d, duplicates %d\n", dedupe, counts[0], counts[1], counts[2],
             counts[md::kDegenerate], counts[md::kDuplicates]);
      rc |= (ok && counts[1] + counts[md::kDegenerate] + counts[md::kDuplicates] == F && (dedupe || !counts[md::kDuplicates])) ? 0 : 8;
    }
    std::vector<int> bad(faces);
    bad[100] = V;
    rc |= mdh_decimate(V, F, verts.data(), bad.data(), nullptr, 0.5, 1, counts, nullptr, nullptr, nullptr, nullptr);
    rc |= counts[md::kStatus] == md::kStatusBadFace ? 0 : 16;
    bad[100] = -1;
    rc |= mdh_decimate(V, F, verts.data(), bad.data(), nullptr, 0.5, 1, counts, nullptr, nullptr, nullptr, nullptr);
    rc |= counts[md::kStatus] == md::kStatusBadFace ? 0 : 16;
    std::vector<float> far(verts);
    far[7] = 1e30f;
    rc |= mdh_decimate(V, F, far.data(), faces.data(), nullptr, 0.5, 1, counts, nullptr, nullptr, nullptr, nullptr);
    rc |= counts[md::kStatus] == md::kStatusBadVertex ? 0 : 32;
    far[7] = -std::numeric_limits<float>::infinity();
    rc |= mdh_decimate(V, F, far.data(), faces.data(), nullptr, 0.5, 1, counts, nullptr, nullptr, nullptr, nullptr);
    rc |= counts[md::kStatus] == md::kStatusBadVertex ? 0 : 32;
    printf("refusals: rc %d\n", rc);
  }
  return rc;
}
#endif
