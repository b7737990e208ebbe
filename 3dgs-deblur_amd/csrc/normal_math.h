// normal_math.h — normals from the rendered depth, the normal-prior loss and the normal smoothness loss (normals.py): the
// depth-normal regularisers of DN-Splatter and of the 2DGS / GOF family (recollected, none of them is part of the
// reference tree), in their cosine form.  Shared by csrc/normals.hip and the host build of
// tests/host_math/normal_host.cpp (TEST INFRASTRUCTURE ONLY; same arrangement as depthprior_math.h).
// Compile with -ffp-contract=off: every float32 operation below rounds on its own.
//
//   inputs   per frame depth_acc, alphas [S,H,W] (the compositor's per-sample sums), intrins fx fy cx cy of the camera
//            the frame was rendered with, prior [H,W,3] or none, guide [H,W,3] or none, prior_weight, smooth_weight,
//            edge_beta >= 0, min_alpha >= 0
//   pixel    d, a = depthprior::sample_mean of the two; has_z = a > min_alpha && d > 0; z = d / a
//   point    P = (rx z, ry z, z), rx = ((u + 0.5) - cx) / fx, ry = ((v + 0.5) - cy) / fy: float32, every operation rounded
//   normal   at an interior pixel (1 <= u <= W - 2, 1 <= v <= H - 2) whose own has_z and that of its four axis
//            neighbours hold: tx = P(u+1,v) - P(u-1,v), ty = P(u,v+1) - P(u,v-1), c = ty x tx, l2 = (c.x c.x + c.y c.y)
//            + c.z c.z; defined iff l2 > 1e-30f (a definition, not a tolerance); n = c / sqrtf(l2).  Camera frame (x right,
//            y down, z forward), facing the camera without a flip.  An undefined pixel holds (0, 0, 0), and the stored
//            value is the record: a pixel has a normal iff a component of it is not 0
//   prior    p has a value iff l = (p.x p.x + p.y p.y) + p.z p.z is > 0 and finite in float32; m = p / sqrtf(l)
//   terms    float64 of the widened float32 values: prior 1 - n.m over the pixels with a normal and a prior value (Np of
//            them); smoothness g_pq (1 - n_p.n_q) over the horizontally and vertically adjacent pairs with two normals
//            (Ns of them, unweighted), g_pq = expf(-(edge_beta * (s / 3))), s = (|dI_r| + |dI_g|) + |dI_b| of the guide,
//            float32; 1 without a guide or with edge_beta = 0
//   loss     prior_weight sum(1 - n.m) / max(Np, 1) + smooth_weight sum g (1 - n_p.n_q) / max(Ns, 1); a term with a zero
//            count is 0 and contributes exact zero gradients
//   chain    float64, gather form, rounded once on store:
//            v_n(p) = -(prior_weight / Np) m_p - (smooth_weight / Ns) (sum over the defined left, right, upper, lower q
//            of g_pq n_q); v_c = (v_n - n (n.v_n)) / sqrt(l2); v_ty = tx x v_c, v_tx = v_c x ty;
//            v_P(q) = v_tx(q - x) - v_tx(q + x) + v_ty(q - y) - v_ty(q + y), each where that neighbour has a normal;
//            v_z = (rx, ry, 1).v_P; then depthprior::chain in depth space.  A pixel without has_z receives exact zeros
#pragma once
#include "depthprior_math.h"

#define GS_NM_HD GS_DP_HD

namespace gs {
namespace normal {

constexpr int kStats = 6;                 // n_defined, Np, sum(1 - n.m), Ns, sum g (1 - n_p.n_q), sum g
constexpr float kMinL2 = 1e-30f;

struct Sums {
  double n_def, np, sp, ns, ss, sg;
};

GS_NM_HD void clear_sums(Sums& m) { m.n_def = m.np = m.sp = m.ns = m.ss = m.sg = 0.0; }

GS_NM_HD void add_sums(Sums& m, const Sums& o) {
  m.n_def += o.n_def; m.np += o.np; m.sp += o.sp; m.ns += o.ns; m.ss += o.ss; m.sg += o.sg;
}

GS_NM_HD bool has_z(float d, float a, float min_alpha) { return a > min_alpha && d > 0.0f; }

GS_NM_HD bool interior(int u, int v, int H, int W) { return u >= 1 && u <= W - 2 && v >= 1 && v <= H - 2; }

// ray coordinate of pixel index i along one axis: pixel centres at + 0.5
GS_NM_HD float ray(int i, float c, float f) { return (((float)i + 0.5f) - c) / f; }

struct Geom {
  float tx[3], ty[3], c[3], l2;
};

// tangents, cross product and its squared length at pixel (u, v) from the z of its left, right, upper and lower neighbour;
// K = fx fy cx cy.  -> whether the normal is defined
GS_NM_HD bool geometry(int u, int v, const float* K, float zl, float zr, float zu, float zd, Geom& g) {
  const float rx = ray(u, K[2], K[0]), rxl = ray(u - 1, K[2], K[0]), rxr = ray(u + 1, K[2], K[0]);
  const float ry = ray(v, K[3], K[1]), ryu = ray(v - 1, K[3], K[1]), ryd = ray(v + 1, K[3], K[1]);
  g.tx[0] = rxr * zr - rxl * zl; g.tx[1] = ry * zr - ry * zl; g.tx[2] = zr - zl;
  g.ty[0] = rx * zd - rx * zu; g.ty[1] = ryd * zd - ryu * zu; g.ty[2] = zd - zu;
  g.c[0] = g.ty[1] * g.tx[2] - g.ty[2] * g.tx[1];
  g.c[1] = g.ty[2] * g.tx[0] - g.ty[0] * g.tx[2];
  g.c[2] = g.ty[0] * g.tx[1] - g.ty[1] * g.tx[0];
  g.l2 = (g.c[0] * g.c[0] + g.c[1] * g.c[1]) + g.c[2] * g.c[2];
  return g.l2 > kMinL2;
}

GS_NM_HD void unit_normal(const Geom& g, float* n) {
  const float r = sqrtf(g.l2);
  n[0] = g.c[0] / r; n[1] = g.c[1] / r; n[2] = g.c[2] / r;
}

// the stored value is the record: (0, 0, 0) is "no normal"
GS_NM_HD bool defined(const float* n) { return n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f; }

// the normal of pixel (u, v) of an H x W frame; d, a: the sample means around it, (row stride `stride`, at (u, v)
// itself).  Zeros where it is not defined
GS_NM_HD void normal_at(const float* d, const float* a, int stride, int u, int v, int H, int W, const float* K,
                        float min_alpha, float* n) {
  n[0] = n[1] = n[2] = 0.0f;
  if (!interior(u, v, H, W)) return;
  if (!(has_z(d[0], a[0], min_alpha) && has_z(d[-1], a[-1], min_alpha) && has_z(d[1], a[1], min_alpha) &&
        has_z(d[-stride], a[-stride], min_alpha) && has_z(d[stride], a[stride], min_alpha)))
    return;
  Geom g;
  if (geometry(u, v, K, d[-1] / a[-1], d[1] / a[1], d[-stride] / a[-stride], d[stride] / a[stride], g)) unit_normal(g, n);
}

// the prior of a pixel -> whether it has a value, and its unit vector
GS_NM_HD bool prior_unit(const float* p, float* m) {
  const float l = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
  m[0] = m[1] = m[2] = 0.0f;
  if (!(l > 0.0f && l < INFINITY)) return false;
  const float r = sqrtf(l);
  m[0] = p[0] / r; m[1] = p[1] / r; m[2] = p[2] / r;
  return true;
}

// g_pq of two adjacent pixels from their guide colours
GS_NM_HD float pair_weight(const float* ip, const float* iq, float edge_beta) {
  const float s = (fabsf(ip[0] - iq[0]) + fabsf(ip[1] - iq[1])) + fabsf(ip[2] - iq[2]);
  return expf(-(edge_beta * (s / 3.0f)));
}

GS_NM_HD double one_minus_dot(const float* x, const float* y) {
  return 1.0 - (((double)x[0] * (double)y[0] + (double)x[1] * (double)y[1]) + (double)x[2] * (double)y[2]);
}

GS_NM_HD void add_defined(Sums& m) { m.n_def += 1.0; }

GS_NM_HD void add_prior(Sums& m, const float* n, const float* unit_prior) {
  m.np += 1.0;
  m.sp += one_minus_dot(n, unit_prior);
}

GS_NM_HD void add_pair(Sums& m, const float* np_, const float* nq, float g) {
  m.ns += 1.0;
  m.ss += (double)g * one_minus_dot(np_, nq);
  m.sg += (double)g;
}

// what the gradient of every pixel of a frame shares
struct Coef {
  double kp, ks, loss;        // prior_weight / Np, smooth_weight / Ns (0 with a zero count)
};

GS_NM_HD Coef finish(const Sums& m, double prior_weight, double smooth_weight) {
  Coef c;
  c.kp = m.np >= 1.0 ? prior_weight / m.np : 0.0;
  c.ks = m.ns >= 1.0 ? smooth_weight / m.ns : 0.0;
  c.loss = (m.np >= 1.0 ? prior_weight * m.sp / m.np : 0.0) + (m.ns >= 1.0 ? smooth_weight * m.ss / m.ns : 0.0);
  return c;
}

// v_n of a pixel with a normal: unit_prior (zeros without a value), pair_sum = sum over its defined neighbours of g_pq n_q (float64)
GS_NM_HD void grad_normal(const Coef& c, const float* unit_prior, const double* pair_sum, double* vn) {
  for (int k = 0; k < 3; ++k) vn[k] = -(c.kp * (double)unit_prior[k]) - c.ks * pair_sum[k];
}

// v_n -> v_tx, v_ty through n = c / |c|, c = ty x tx
GS_NM_HD void grad_tangents(const Geom& g, const float* n, const double* vn, double* vtx, double* vty) {
  const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
  const double dot = (n0 * vn[0] + n1 * vn[1]) + n2 * vn[2];
  const double r = ::sqrt((double)g.l2);
  const double vc[3] = {(vn[0] - n0 * dot) / r, (vn[1] - n1 * dot) / r, (vn[2] - n2 * dot) / r};
  const double tx[3] = {(double)g.tx[0], (double)g.tx[1], (double)g.tx[2]};
  const double ty[3] = {(double)g.ty[0], (double)g.ty[1], (double)g.ty[2]};
  vty[0] = tx[1] * vc[2] - tx[2] * vc[1];
  vty[1] = tx[2] * vc[0] - tx[0] * vc[2];
  vty[2] = tx[0] * vc[1] - tx[1] * vc[0];
  vtx[0] = vc[1] * ty[2] - vc[2] * ty[1];
  vtx[1] = vc[2] * ty[0] - vc[0] * ty[2];
  vtx[2] = vc[0] * ty[1] - vc[1] * ty[0];
}

// v_P of pixel (u, v) -> v_z
GS_NM_HD double grad_z(int u, int v, const float* K, const double* vP) {
  return ((double)ray(u, K[2], K[0]) * vP[0] + (double)ray(v, K[3], K[1]) * vP[1]) + vP[2];
}

}  // namespace normal
}  // namespace gs
