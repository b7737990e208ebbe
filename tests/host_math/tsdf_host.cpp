// TEST INFRASTRUCTURE ONLY: csrc/tsdf_math.h compiled for the host (tests/test_tsdf_host.py).  The projection, the depth
// test, the update, the tetrahedra, the triangle table and the vertex rule are the kernels'; voxels and samples are visited
// one after the other here.  With -DTSDF_HOST_MAIN the file is a program of its own that runs the small cases (built with
// -fsanitize=address,undefined by the test).
#include "tsdf_math.h"

#include <vector>

namespace ts = gs::tsdf;

extern "C" {

int tsh_frames_per_launch() { return ts::kFramesPerLaunch; }
int tsh_dims_ok(int nx, int ny, int nz) { return ts::dims_ok(nx, ny, nz) ? 1 : 0; }
int tsh_tet_corner(int tet, int n) { return ts::tet_corner(tet, n); }
int tsh_tet_odd(int tet) { return ts::tet_odd(tet); }
int tsh_edge_type_of_code(int code) { return ts::edge_type_of_code(code); }
int tsh_edge_code_of_type(int type) { return ts::edge_code_of_type(type); }
int tsh_case_triangles(int m) { return ts::case_triangles(m); }
void tsh_case_triangle(int m, int odd, int tri, int* ea, int* eb) { ts::case_triangle(m, odd, tri, ea, eb); }

// the arguments of gs_tsdf_integrate, host pointers
int tsh_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float* tsdf, float* weight,
                  float* color, int B, int H, int W, const float* depth, const float* viewmats, const float* intrins,
                  const float* color_images, const float* weight_images, float trunc, float depth_min, float depth_max,
                  float max_weight) {
  if (!ts::dims_ok(nx, ny, nz) || B < 0 || H < 1 || W < 1) return 1;
  const size_t pixels = (size_t)H * W;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const size_t s = ((size_t)k * ny + j) * nx + i;
        const float x = ts::sample_coord(ox, voxel_size, i), y = ts::sample_coord(oy, voxel_size, j),
                    z = ts::sample_coord(oz, voxel_size, k);
        for (int b = 0; b < B; ++b) {
          ts::Camera cam;
          ts::load_camera(viewmats + (size_t)b * 16, intrins + (size_t)b * 4, cam);
          float zc, val;
          int px, py;
          if (!ts::project(cam, x, y, z, W, H, &zc, &px, &py)) continue;
          const size_t p = (size_t)b * pixels + (size_t)py * W + px;
          const float w = weight_images ? weight_images[p] : 1.0f;
          if (!ts::depth_sample(depth[p], w, zc, trunc, depth_min, depth_max, &val)) continue;
          const float Wt = weight[s], Wn = Wt + w;
          tsdf[s] = ts::blend(tsdf[s], Wt, val, w, Wn);
          if (color)
            for (int c = 0; c < 3; ++c) color[s * 3 + c] = ts::blend(color[s * 3 + c], Wt, color_images[p * 3 + c], w, Wn);
          weight[s] = fminf(Wn, max_weight);
        }
      }
  return 0;
}

// count (verts == NULL: only counts[0] = V, counts[1] = F) or emit; the arguments of gs_tsdf_mesh_count / _emit
int tsh_mesh(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf, const float* weight,
             const float* color, float level, float min_weight, int* counts, float* verts, int* faces, float* colors) {
  if (!ts::dims_ok(nx, ny, nz)) return 1;
  const ts::Grid g = {nx, ny, nz, level, min_weight};
  const size_t n = (size_t)nx * ny * nz;
  std::vector<unsigned char> edges(n);
  std::vector<unsigned> first(n);
  unsigned V = 0, F = 0;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const size_t s = ts::linear(g, i, j, k);
        edges[s] = (unsigned char)ts::sample_edges(g, tsdf, weight, i, j, k);
        first[s] = V;
        V += (unsigned)ts::popcount7(edges[s]);
        F += (unsigned)ts::cell_faces(g, tsdf, weight, i, j, k);
      }
  counts[0] = (int)V; counts[1] = (int)F;
  if (!verts) return 0;
  const float origin[3] = {ox, oy, oz};
  unsigned at = 0;
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const size_t s = ts::linear(g, i, j, k);
        for (int type = 0; type < ts::kEdgeTypes; ++type) {
          if (!((edges[s] >> type) & 1)) continue;
          const size_t v = first[s] + (unsigned)ts::popcount7(edges[s] & ((1 << type) - 1));
          ts::edge_vertex(g, tsdf, colors ? color : nullptr, origin, voxel_size, i, j, k, type, verts + v * 3,
                          colors ? colors + v * 3 : nullptr);
        }
        const int nf = ts::cell_faces(g, tsdf, weight, i, j, k);
        if (!nf) continue;
        const int cm = ts::cell_mask(g, tsdf, i, j, k);
        for (int tet = 0; tet < 6; ++tet) {
          const int m = ts::tet_case(cm, tet);
          for (int tri = 0; tri < ts::case_triangles(m); ++tri) {
            int ea[3], eb[3];
            ts::case_triangle(m, ts::tet_odd(tet), tri, ea, eb);
            for (int e = 0; e < 3; ++e) {
              const int ca = ts::tet_corner(tet, ea[e]), cb = ts::tet_corner(tet, eb[e]);
              const size_t owner = ts::linear(g, i + (ca & 1), j + ((ca >> 1) & 1), k + (ca >> 2));
              const int type = ts::edge_type_of_code(ca ^ cb);
              faces[(size_t)at * 3 + e] = (int)(first[owner] + (unsigned)ts::popcount7(edges[owner] & ((1 << type) - 1)));
            }
            ++at;
          }
        }
      }
  return at == F ? 0 : 2;
}

}  // extern "C"

#ifdef TSDF_HOST_MAIN
#include <stdio.h>

// the small cases under the sanitizers: a 33 x 17 x 9 volume fused from 5 ring cameras with NaN / zero / weightless
// pixels, and the mesh of it and of a sphere in an 11 x 9 x 7 volume
int main() {
  const int nx = 33, ny = 17, nz = 9, B = 5, H = 32, W = 48;
  const size_t n = (size_t)nx * ny * nz, pixels = (size_t)H * W;
  std::vector<float> tsdf(n, 1.0f), weight(n, 0.0f), color(n * 3, 0.0f);
  std::vector<float> depth(B * pixels), cimg(B * pixels * 3), wimg(B * pixels, 1.0f), views(B * 16, 0.0f), intr(B * 4);
  for (int b = 0; b < B; ++b) {
    const float a = 0.1f + 6.2831853f * (float)b / (float)B, c = cosf(a), s = sinf(a);
    // camera at 2.5 (c, s, 0) looking at the origin: right = (-s, c, 0), down = (0, 0, -1), forward = (-c, -s, 0)
    const float R[9] = {-s, c, 0.0f, 0.0f, 0.0f, -1.0f, -c, -s, 0.0f};
    const float eye[3] = {2.5f * c, 2.5f * s, 0.0f};
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) views[b * 16 + r * 4 + q] = R[r * 3 + q];
      views[b * 16 + r * 4 + 3] = -(R[r * 3] * eye[0] + R[r * 3 + 1] * eye[1] + R[r * 3 + 2] * eye[2]);
    }
    views[b * 16 + 15] = 1.0f;
    intr[b * 4] = 40.0f; intr[b * 4 + 1] = 40.0f; intr[b * 4 + 2] = 24.0f; intr[b * 4 + 3] = 16.0f;
    for (size_t p = 0; p < pixels; ++p) {
      const float u = (float)(p % W) / W, v = (float)(p / W) / H;
      depth[b * pixels + p] = 2.5f + 0.25f * sinf(3.0f * u + b) * cosf(2.0f * v);
      for (int q = 0; q < 3; ++q) cimg[(b * pixels + p) * 3 + q] = 0.5f + 0.5f * sinf(4.0f * u + q + b);
    }
  }
  depth[5] = NAN; depth[6] = INFINITY; depth[7] = 0.0f; wimg[pixels + 9] = 0.0f;
  int rc = tsh_integrate(nx, ny, nz, -1.0f, -0.5f, -0.25f, 0.0625f, tsdf.data(), weight.data(), color.data(), B, H, W,
                         depth.data(), views.data(), intr.data(), cimg.data(), wimg.data(), 0.25f, 0.0f, 2.7f, 3.0f);
  size_t touched = 0;
  for (size_t s = 0; s < n; ++s) touched += weight[s] > 0.0f;
  int counts[2] = {0, 0};
  rc |= tsh_mesh(nx, ny, nz, -1.0f, -0.5f, -0.25f, 0.0625f, tsdf.data(), weight.data(), color.data(), 0.0f, 0.0f, counts,
                 nullptr, nullptr, nullptr);
  std::vector<float> verts((size_t)counts[0] * 3 + 1), cols((size_t)counts[0] * 3 + 1);
  std::vector<int> faces((size_t)counts[1] * 3 + 1);
  rc |= tsh_mesh(nx, ny, nz, -1.0f, -0.5f, -0.25f, 0.0625f, tsdf.data(), weight.data(), color.data(), 0.0f, 0.0f, counts,
                 verts.data(), faces.data(), cols.data());
  printf("fused: touched %zu of %zu, V %d, F %d\n", touched, n, counts[0], counts[1]);
  const int mx = 11, my = 9, mz = 7;
  std::vector<float> f((size_t)mx * my * mz), w((size_t)mx * my * mz, 1.0f);
  for (int k = 0; k < mz; ++k)
    for (int j = 0; j < my; ++j)
      for (int i = 0; i < mx; ++i)
        f[((size_t)k * my + j) * mx + i] = sqrtf((i - 5.2f) * (i - 5.2f) + (j - 4.1f) * (j - 4.1f) + (k - 3.3f) * (k - 3.3f)) - 2.6f;
  int c2[2] = {0, 0};
  rc |= tsh_mesh(mx, my, mz, 1.0f, 2.0f, 3.0f, 1.0f, f.data(), w.data(), nullptr, 0.0f, 0.0f, c2, nullptr, nullptr, nullptr);
  std::vector<float> v2((size_t)c2[0] * 3 + 1);
  std::vector<int> f2((size_t)c2[1] * 3 + 1);
  rc |= tsh_mesh(mx, my, mz, 1.0f, 2.0f, 3.0f, 1.0f, f.data(), w.data(), nullptr, 0.0f, 0.0f, c2, v2.data(), f2.data(), nullptr);
  for (int q = 0; q < c2[1] * 3; ++q) rc |= (f2[q] < 0 || f2[q] >= c2[0]) ? 4 : 0;
  printf("sphere: V %d, F %d, status %d\n", c2[0], c2[1], rc);
  return (rc == 0 && touched > 0 && counts[1] > 0 && c2[0] - c2[1] / 2 == 2) ? 0 : 1;
}
#endif
