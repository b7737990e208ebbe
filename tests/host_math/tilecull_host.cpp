// Host build of csrc/tilecull_math.h — TEST INFRASTRUCTURE ONLY (tests/test_slicefront_host.py, tests/test_gpu_slicefront.py).
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I3dgs-deblur_amd/csrc tests/host_math/tilecull_host.cpp -o libtilecull_host.so
// Runs the header's ellipse test over the tile box of every record, exactly as the kernels call it: the per-tile form
// (tile_hit) and the per-row form (row_span + span_tiles over the whole box row, what the exact count walks).
//
// -DTILECULL_MAIN adds a main() that runs a seeded fuzz stand-alone (for a sanitizer build of the header's host code):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -DTILECULL_MAIN -I... tilecull_host.cpp -o tilecull_fuzz
#include <stdint.h>
#include <string.h>
#include "tilecull_math.h"

using namespace gs;

namespace {

inline void rec_box(const float* rec, int& x0, int& y0, int& x1, int& y1) {
  uint32_t lo, hi;
  memcpy(&lo, rec + 10, 4); memcpy(&hi, rec + 11, 4);
  x0 = (int)(lo & 0xFFFFu); y0 = (int)(lo >> 16); x1 = (int)(hi & 0xFFFFu); y1 = (int)(hi >> 16);
}

// the ellipse of record i as slice_counts_exact_kernel builds it (swept fields after make_ellipse)
inline Ellipse rec_ellipse(const float* rec, int sweep, const float* pv, float t_min, float t_max, float rs) {
  Ellipse e = make_ellipse(rec);
  e.pvx = e.pvy = e.st0 = e.st1 = e.srs = 0.f;
  if (sweep) { e.pvx = pv[0]; e.pvy = pv[1]; e.st0 = fminf(t_min, t_max); e.st1 = fmaxf(t_min, t_max); e.srs = rs; }
  return e;
}

}  // namespace

extern "C" {

// out[off[i] + (ty - y0) * w + (tx - x0)] = 1 when tile (tx, ty) of record i's box passes the ellipse test, else 0.
// by_row = 0: tile_hit<SWEEP> per tile; by_row = 1: span_tiles(row_span<SWEEP>) over the whole box row.
// off[i] = sum of the box areas of the records before i (off has n + 1 entries).  pix_vel [n, 2] (sweep only).
int tc_hits(int n, const float* recs, int W, int H, int sweep, const float* pix_vel, float t_min, float t_max, float rs,
            int by_row, const long long* off, unsigned char* out) {
  if (n < 0 || !recs || !off || !out || (sweep && !pix_vel)) return 1;
  for (int i = 0; i < n; ++i) {
    const float* rec = recs + (size_t)i * kRecFloats;
    int x0, y0, x1, y1;
    rec_box(rec, x0, y0, x1, y1);
    const int w = x1 - x0, h = y1 - y0;
    if (w <= 0 || h <= 0) { if (off[i + 1] != off[i]) return 2; continue; }
    if (off[i + 1] - off[i] != (long long)w * h) return 2;
    const Ellipse e = rec_ellipse(rec, sweep, sweep ? pix_vel + 2 * (size_t)i : nullptr, t_min, t_max, rs);
    unsigned char* o = out + off[i];
    for (int ty = y0; ty < y1; ++ty) {
      if (by_row) {
        int t0, t1;
        if (sweep) span_tiles(e, row_span<true>(e, ty, H), x0, x1, t0, t1);
        else span_tiles(e, row_span<false>(e, ty, H), x0, x1, t0, t1);
        for (int tx = x0; tx < x1; ++tx) o[(size_t)(ty - y0) * w + (tx - x0)] = (tx >= t0 && tx < t1) ? 1 : 0;
      } else {
        for (int tx = x0; tx < x1; ++tx)
          o[(size_t)(ty - y0) * w + (tx - x0)] =
              (sweep ? tile_hit<true>(e, tx, ty, W, H) : tile_hit<false>(e, tx, ty, W, H)) ? 1 : 0;
      }
    }
  }
  return 0;
}

// the derived numbers of record i (tau with its slack, ustar, vext, vstar): out[4 * i ..]
int tc_derived(int n, const float* recs, float* out) {
  for (int i = 0; i < n; ++i) {
    const Ellipse e = make_ellipse(recs + (size_t)i * kRecFloats);
    out[4 * i] = e.tau; out[4 * i + 1] = e.ustar; out[4 * i + 2] = e.vext; out[4 * i + 3] = e.vstar;
  }
  return 0;
}

}  // extern "C"

#ifdef TILECULL_MAIN
// Stand-alone fuzz: the distribution of tests/test_slicefront_host.py (major axis 0.3 .. 6000 px, anisotropy up to 2e4
// with the minor axis floored at 0.3 px, any angle, centres on / just off / far off screen, three opacity bands,
// 2048 x 200).  Checks, static and swept: the per-tile and the per-row form agree; no tile with a pixel centre of
// alpha >= 1/255 (float64, every pixel of the tile, the swept form minimised over its time interval) is culled.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double urand() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}
double logu(double lo, double hi) { return lo * exp(urand() * log(hi / lo)); }

bool strict_tile(const float* rec, int tx, int ty, int W, int H, int sweep, const float* pv, double t0, double t1, double rs) {
  const double gx = rec[0], gy = rec[1], a = rec[2], b = rec[3], c = rec[4], o = rec[5];
  for (int py = ty * 16; py < ty * 16 + 16 && py < H; ++py)
    for (int px = tx * 16; px < tx * 16 + 16 && px < W; ++px) {
      double dx = px + 0.5 - gx, dy = py + 0.5 - gy;
      if (sweep) {
        const double tr = ((py + 0.5) / H - 0.5) * rs, lo = t0 + tr, hi = t1 + tr, vx = pv[0], vy = pv[1];
        const double q2 = 0.5 * (a * vx * vx + c * vy * vy) + b * vx * vy;
        const double q1 = a * dx * vx + c * dy * vy + b * (dx * vy + dy * vx);
        double t = q2 > 0 ? q1 / (2 * q2) : lo;
        t = t < lo ? lo : (t > hi ? hi : t);
        double best = 1e300;
        for (double tt : {t, lo, hi}) {
          const double ex = dx - tt * vx, ey = dy - tt * vy, s = 0.5 * (a * ex * ex + c * ey * ey) + b * ex * ey;
          if (s < best) best = s;
        }
        if (o * exp(-best) >= 1.0 / 255.0) return true;
      } else if (o * exp(-(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy)) >= 1.0 / 255.0) return true;
    }
  return false;
}
}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 20000;
  const int W = 2048, H = 200, TX = 128, TY = 13;
  std::vector<float> recs((size_t)n * kRecFloats, 0.f), pv((size_t)n * 2);
  std::vector<long long> off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    float* r = &recs[(size_t)i * kRecFloats];
    const double s1 = logu(0.3, 6000.0), an = logu(1.0, 2e4), s2 = fmax(s1 / an, 0.3), th = urand() * 6.283185307179586;
    const double cs = cos(th), sn = sin(th), l1 = s1 * s1, l2 = s2 * s2;
    const double cxx = cs * cs * l1 + sn * sn * l2, cxy = cs * sn * (l1 - l2), cyy = sn * sn * l1 + cs * cs * l2;
    const double det = l1 * l2;
    const int where = (int)(urand() * 3);
    double gx = urand() * W, gy = urand() * H;
    if (where == 1) { gx = urand() < 0.5 ? -urand() * 40 : W + urand() * 40; gy = urand() < 0.5 ? -urand() * 40 : H + urand() * 40; }
    if (where == 2) { gx += (urand() < 0.5 ? -2e4 : 2e4); gy += (urand() < 0.5 ? -2e4 : 2e4) * (urand() < 0.5); }
    const int band = (int)(urand() * 3);
    const double op = band == 0 ? (1.0 / 255.0) * (1.0 + 0.05 * urand()) : (band == 1 ? 0.999 + 0.001 * urand() : urand());
    r[0] = (float)gx; r[1] = (float)gy; r[2] = (float)(cyy / det); r[3] = (float)(-cxy / det); r[4] = (float)(cxx / det);
    r[5] = (float)op;
    pv[2 * i] = (float)((urand() - 0.5) * 800); pv[2 * i + 1] = (float)((urand() - 0.5) * 800);
    const double rad = ceil(3 * s1) + 400 * (1.0 / 60 + 1.0 / 60);           // covers the swept offsets below
    auto cl = [](double v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); };
    const int x0 = cl(floor((gx - rad) / 16), TX), x1 = cl(floor((gx + rad) / 16) + 1, TX);
    const int y0 = cl(floor((gy - rad) / 16), TY), y1 = cl(floor((gy + rad) / 16) + 1, TY);
    const uint32_t lo = (uint32_t)x0 | ((uint32_t)y0 << 16), hi = (uint32_t)x1 | ((uint32_t)y1 << 16);
    memcpy(r + 10, &lo, 4); memcpy(r + 11, &hi, 4);
    off[i + 1] = off[i] + (x1 > x0 && y1 > y0 ? (long long)(x1 - x0) * (y1 - y0) : 0);
  }
  std::vector<unsigned char> bt(off[n] + 1), br(off[n] + 1);
  int bad = 0;
  for (int sweep = 0; sweep < 2; ++sweep) {
    const float t0 = sweep ? -1.f / 120 : 0.f, t1 = sweep ? 1.f / 120 : 0.f, rs = sweep ? 1.f / 30 : 0.f;
    if (tc_hits(n, recs.data(), W, H, sweep, pv.data(), t0, t1, rs, 0, off.data(), bt.data())) return 2;
    if (tc_hits(n, recs.data(), W, H, sweep, pv.data(), t0, t1, rs, 1, off.data(), br.data())) return 2;
    long long kept = 0, strict = 0, culled_strict = 0, forms = 0;
    for (int i = 0; i < n; ++i) {
      const float* r = &recs[(size_t)i * kRecFloats];
      int x0, y0, x1, y1;
      rec_box(r, x0, y0, x1, y1);
      if (off[i + 1] == off[i]) continue;
      // the exhaustive pixel check is what costs: every 4th record (every 16th when swept)
      const bool check = i % (sweep ? 16 : 4) == 0;
      for (int ty = y0; ty < y1; ++ty)
        for (int tx = x0; tx < x1; ++tx) {
          const size_t k = off[i] + (size_t)(ty - y0) * (x1 - x0) + (tx - x0);
          forms += bt[k] != br[k];
          if (!check) continue;
          const bool s = strict_tile(r, tx, ty, W, H, sweep, &pv[2 * i], t0, t1, rs);
          kept += bt[k]; strict += s; culled_strict += s && !bt[k];
        }
    }
    printf("%s: %d ellipses, %lld pairs, checked: kept %lld strict %lld, strict pairs culled %lld, tile/row forms differ %lld\n",
           sweep ? "swept" : "static", n, off[n], kept, strict, culled_strict, forms);
    bad += culled_strict != 0 || forms != 0;
  }
  return bad ? 1 : 0;
}
#endif
