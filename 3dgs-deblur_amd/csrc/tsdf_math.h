// tsdf_math.h — TSDF fusion of depth maps and marching-tetrahedra mesh extraction (tsdf.py).  Shared by csrc/tsdf.hip and
// the host build of tests/host_math/tsdf_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as knn_math.h).
// Compile with -ffp-contract=off: every float32 operation below rounds on its own.
//
// VOLUME   tsdf, weight [nz,ny,nx], color [nz,ny,nx,3] float32, x fastest; sample (i, j, k) sits at
//          origin + voxel_size * (i, j, k), each coordinate origin_a + voxel_size * float(index).
// UPDATE   per voxel, frames in index order:
//   project  p = R x + t with p_r = ((r0 * x + r1 * y) + r2 * z) + t_r, z = p.z; skip the frame if z <= 0
//            u = (fx * p.x) / z + cx, v = (fy * p.y) / z + cy; px = floor(u), py = floor(v) (pixel centres at +0.5);
//            skip unless 0 <= u < W and 0 <= v < H
//   depth    D = depth[py, px], w = weights[py, px] (1 without weights); skip unless D is finite,
//            depth_min < D <= depth_max and w > 0; sdf = D - z; skip if sdf < -trunc; val = min(1, sdf / trunc)
//   update   Wn = W + w; tsdf = (tsdf * W + val * w) / Wn; every colour channel likewise; W = min(Wn, max_weight)
// MESH     marching tetrahedra on the Kuhn split: a cell is cut into the six tetrahedra along its monotone corner paths
//          000 -> 111, one per order of the axes, lexicographic: xyz, xzy, yxz, yzx, zxy, zyx; corners c0 = 000,
//          c1 = c0 + e_a, c2 = c1 + e_b, c3 = 111.  A corner is inside when tsdf < level; a cell is used when all 8
//          corners have weight > min_weight.
//   lone corner a (one inside or one outside), others o0 < o1 < o2 in path order: triangle (a-o0, a-o1, a-o2)
//   inside a < b, outside c < d: quad (ac, ad, bd, bc) split as (ac, ad, bd), (ac, bd, bc)
//   either way reversed (entries 1 and 2 swapped) where the normal would point towards decreasing tsdf: a fixed parity
//   per case (kFlipEven, for the even orders xyz, yzx, zxy; the odd orders take the opposite)
//   vertices live on the 7 edges a sample owns (+x, +y, +z, +xy, +xz, +yz, +xyz: types 0..6), one per crossed edge
//   that belongs to a used cell, at pa + t (pb - pa), t = (level - fa) / (fb - fa), a the owner; colour likewise
//   order    vertices by (owner's linear index k ny nx + j nx + i, edge type); faces by (cell's linear index — that of
//            its lower corner —, tetrahedron, triangle)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GS_TSDF_HD __host__ __device__ __forceinline__
#else
#define GS_TSDF_HD inline
#endif

namespace gs {
namespace tsdf {

constexpr int kFramesPerLaunch = 16;            // frames one launch of the integrate kernel applies
constexpr int kMinDim = 2, kMaxDim = 1024;
constexpr long long kMaxVoxels = 1LL << 30;
constexpr int kMaxImageDim = 16384;
constexpr int kEdgeTypes = 7;
constexpr int kMaxCellFaces = 12;

GS_TSDF_HD bool dims_ok(int nx, int ny, int nz) {
  if (nx < kMinDim || ny < kMinDim || nz < kMinDim || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim) return false;
  return (long long)nx * ny * nz <= kMaxVoxels;
}

// ---- integration ------------------------------------------------------------------------------------------------------
struct Camera {
  float r[12];                 // rows 0..2 of the world-to-camera matrix: r[4 * row + col], col 3 the translation
  float fx, fy, cx, cy;
};

GS_TSDF_HD void load_camera(const float* viewmat16, const float* intrin4, Camera& c) {
  for (int q = 0; q < 12; ++q) c.r[q] = viewmat16[q];
  c.fx = intrin4[0]; c.fy = intrin4[1]; c.cx = intrin4[2]; c.cy = intrin4[3];
}

GS_TSDF_HD float sample_coord(float origin, float voxel_size, int index) { return origin + voxel_size * (float)index; }

// camera-space z and the pixel of a world point; false: behind the camera or outside the image
GS_TSDF_HD bool project(const Camera& c, float x, float y, float z, int W, int H, float* zc, int* px, int* py) {
  const float pxc = ((c.r[0] * x + c.r[1] * y) + c.r[2] * z) + c.r[3];
  const float pyc = ((c.r[4] * x + c.r[5] * y) + c.r[6] * z) + c.r[7];
  const float pzc = ((c.r[8] * x + c.r[9] * y) + c.r[10] * z) + c.r[11];
  if (!(pzc > 0.0f)) return false;
  const float u = (c.fx * pxc) / pzc + c.cx;
  const float v = (c.fy * pyc) / pzc + c.cy;
  if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) return false;
  *zc = pzc; *px = (int)floorf(u); *py = (int)floorf(v);
  return true;
}

// the depth test; val: the truncated signed distance in units of trunc
GS_TSDF_HD bool depth_sample(float D, float w, float z, float trunc, float depth_min, float depth_max, float* val) {
  if (!(fabsf(D) <= 3.4028234663852886e38f)) return false;        // NaN, +-inf
  if (!(D > depth_min && D <= depth_max && w > 0.0f)) return false;
  const float sdf = D - z;
  if (sdf < -trunc) return false;
  *val = fminf(1.0f, sdf / trunc);
  return true;
}

GS_TSDF_HD float blend(float old, float W, float val, float w, float Wn) { return (old * W + val * w) / Wn; }

// ---- marching tetrahedra ----------------------------------------------------------------------------------------------
// corner codes: bit 0 = +x, bit 1 = +y, bit 2 = +z
GS_TSDF_HD int tet_odd(int tet) { return (0x26 >> tet) & 1; }           // xzy, yxz, zyx are odd orders of the axes

// corner n (0..3) of tetrahedron tet (0..5) as a corner code
GS_TSDF_HD int tet_corner(int tet, int n) {
  const int a = tet >> 1;
  const int lo = a == 0 ? 1 : 0, hi = a == 2 ? 1 : 2;
  const int b = (tet & 1) ? hi : lo;
  const int c1 = 1 << a, c2 = c1 | (1 << b);
  return n == 0 ? 0 : (n == 1 ? c1 : (n == 2 ? c2 : 7));
}

GS_TSDF_HD int edge_type_of_code(int code) { return (int)((0x65423100u >> (4 * code)) & 15u); }
GS_TSDF_HD int edge_code_of_type(int type) { return (int)((0x7653421u >> (4 * type)) & 15u); }

// the 4-bit case of a tetrahedron from the cell's 8-bit inside mask (bit n: corner n of the path is inside)
GS_TSDF_HD int tet_case(int cell_mask, int tet) {
  int m = 0;
  for (int n = 0; n < 4; ++n) m |= ((cell_mask >> tet_corner(tet, n)) & 1) << n;
  return m;
}

GS_TSDF_HD int case_triangles(int m) {
  const int n = (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1);
  return (n == 0 || n == 4) ? 0 : (n == 2 ? 2 : 1);
}

constexpr unsigned kFlipEven = 0x4D24u;         // bit m: case m of an even order is emitted reversed

// triangle tri of case m: its three edges as pairs of path corners ea[q] < eb[q], already oriented
GS_TSDF_HD void case_triangle(int m, int odd, int tri, int ea[3], int eb[3]) {
  int in[4], out[4], ni = 0, no = 0;
  for (int n = 0; n < 4; ++n) {
    if ((m >> n) & 1) in[ni++] = n; else out[no++] = n;
  }
  int p[3], q[3];
  if (ni == 1) {
    for (int e = 0; e < 3; ++e) { p[e] = in[0]; q[e] = out[e]; }
  } else if (ni == 3) {
    for (int e = 0; e < 3; ++e) { p[e] = out[0]; q[e] = in[e]; }
  } else {
    const int a = in[0], b = in[1], c = out[0], d = out[1];
    p[0] = a; q[0] = c;
    if (tri == 0) { p[1] = a; q[1] = d; p[2] = b; q[2] = d; } else { p[1] = b; q[1] = d; p[2] = b; q[2] = c; }
  }
  if ((int)((kFlipEven >> m) & 1u) != odd) {
    int t = p[1]; p[1] = p[2]; p[2] = t;
    t = q[1]; q[1] = q[2]; q[2] = t;
  }
  for (int e = 0; e < 3; ++e) { ea[e] = p[e] < q[e] ? p[e] : q[e]; eb[e] = p[e] < q[e] ? q[e] : p[e]; }
}

struct Grid {
  int nx, ny, nz;
  float level, min_weight;
};

GS_TSDF_HD size_t linear(const Grid& g, int i, int j, int k) { return ((size_t)k * g.ny + j) * g.nx + i; }

GS_TSDF_HD bool is_cell(const Grid& g, int i, int j, int k) {
  return i >= 0 && j >= 0 && k >= 0 && i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1;
}

GS_TSDF_HD bool cell_used(const Grid& g, const float* weight, int i, int j, int k) {
  if (!is_cell(g, i, j, k)) return false;
  bool used = true;
  for (int c = 0; c < 8; ++c) used = used && weight[linear(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] > g.min_weight;
  return used;
}

// the cell's inside mask by corner code (the cell must exist)
GS_TSDF_HD int cell_mask(const Grid& g, const float* tsdf, int i, int j, int k) {
  int m = 0;
  for (int c = 0; c < 8; ++c) m |= (tsdf[linear(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] < g.level ? 1 : 0) << c;
  return m;
}

GS_TSDF_HD int mask_faces(int cell_mask8) {
  if (cell_mask8 == 0 || cell_mask8 == 255) return 0;
  int n = 0;
  for (int t = 0; t < 6; ++t) n += case_triangles(tet_case(cell_mask8, t));
  return n;
}

// faces of the cell whose lower corner is the sample (0 when it is no cell or not used)
GS_TSDF_HD int cell_faces(const Grid& g, const float* tsdf, const float* weight, int i, int j, int k) {
  if (!is_cell(g, i, j, k)) return 0;
  const int m = cell_mask(g, tsdf, i, j, k);
  if (m == 0 || m == 255) return 0;
  return cell_used(g, weight, i, j, k) ? mask_faces(m) : 0;
}

// the 7-bit mask of the owned edges that carry a vertex: crossed, and an edge of at least one used cell
GS_TSDF_HD int sample_edges(const Grid& g, const float* tsdf, const float* weight, int i, int j, int k) {
  const bool own = tsdf[linear(g, i, j, k)] < g.level;
  int mask = 0;
  for (int type = 0; type < kEdgeTypes; ++type) {
    const int d = edge_code_of_type(type);
    const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
    if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz) continue;
    if ((tsdf[linear(g, i + dx, j + dy, k + dz)] < g.level) == own) continue;
    // the cells that hold the edge: one step back along every axis the edge does not run along
    bool any = false;
    for (int az = 0; az <= 1 - dz; ++az)
      for (int ay = 0; ay <= 1 - dy; ++ay)
        for (int ax = 0; ax <= 1 - dx; ++ax) any = any || cell_used(g, weight, i - ax, j - ay, k - az);
    if (any) mask |= 1 << type;
  }
  return mask;
}

GS_TSDF_HD int popcount7(int m) {
  int n = 0;
  for (int b = 0; b < kEdgeTypes; ++b) n += (m >> b) & 1;
  return n;
}

GS_TSDF_HD float edge_t(float level, float fa, float fb) { return (level - fa) / (fb - fa); }
GS_TSDF_HD float lerp(float a, float b, float t) { return a + t * (b - a); }

// vertex (and colour) of the edge of `type` owned by sample (i, j, k)
GS_TSDF_HD void edge_vertex(const Grid& g, const float* tsdf, const float* color, const float origin[3], float voxel_size,
                            int i, int j, int k, int type, float vert[3], float col[3]) {
  const int d = edge_code_of_type(type);
  const int i2 = i + (d & 1), j2 = j + ((d >> 1) & 1), k2 = k + (d >> 2);
  const size_t a = linear(g, i, j, k), b = linear(g, i2, j2, k2);
  const float t = edge_t(g.level, tsdf[a], tsdf[b]);
  vert[0] = lerp(sample_coord(origin[0], voxel_size, i), sample_coord(origin[0], voxel_size, i2), t);
  vert[1] = lerp(sample_coord(origin[1], voxel_size, j), sample_coord(origin[1], voxel_size, j2), t);
  vert[2] = lerp(sample_coord(origin[2], voxel_size, k), sample_coord(origin[2], voxel_size, k2), t);
  if (color) {
    for (int c = 0; c < 3; ++c) col[c] = lerp(color[a * 3 + c], color[b * 3 + c], t);
  }
}

}  // namespace tsdf
}  // namespace gs
