"""Plain numpy / float64 restatement of the slice front end of csrc/binning.hip (TEST INFRASTRUCTURE ONLY; shares no code
with the kernels).  Contracts: include/gsdeblur.h and csrc/tilecull_math.h.

Ellipse test.  A record holds (gx, gy, a, b, c, o) as float32; everything below is evaluated in float64 from those values.
sigma(dx, dy) = (a dx^2 + c dy^2) / 2 + b dx dy, alpha = o exp(-sigma); tile (tx, ty) holds the pixel centres
16 tx + 0.5 .. 16 tx + 15.5 (likewise in y).

  strict   some pixel centre of the tile INSIDE the image has alpha >= 1/255: the pairs the cull must keep
  loose    the float64 minimum of sigma over the continuous pixel-centre rectangle of the tile (rows clipped to H - 0.5,
           the last tile column at full width), the rectangle grown by 4e-3 + 4e-6 (|gx| + u_extent) pixels, is at most
           1.003 ln(255 o) + 3e-3: twice the slack tilecull_math.h documents.  Only for conics with det >= 1e-3 a c: below
           that the float32 determinant is noise and the kernel keeps everything
  swept    the centre is xy + t pix_vel, t in [t_min + tr(y), t_max + tr(y)], tr(y) = ((y + 0.5) / H - 0.5) T_ro.  strict:
           per pixel, sigma minimised over t in closed form (a clamped 1-D quadratic).  loose: the kernel documents the x
           and y offsets of a tile row as INDEPENDENT intervals (a box around the swept segment), so the rectangle is
           widened by that box, taken over the rows of the tile row, and grown by twice the documented sweep slack
           1e-3 + 1e-5 (|t_lo| + |t_hi|) (|vx| + |vy|) on top of the static growth
"""
import numpy as np

TILE = 16
ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = np.float32(0.999)
REC = 16


# ---- records ----------------------------------------------------------------------------------------------------------
def boxes_of(rec):
    lo = np.ascontiguousarray(rec[:, 10]).view(np.uint32).astype(np.int64)
    hi = np.ascontiguousarray(rec[:, 11]).view(np.uint32).astype(np.int64)
    return lo & 0xFFFF, lo >> 16, hi & 0xFFFF, hi >> 16


def make_records(xy, conic, op, box):
    """records [n, 16] float32 with the fields the front end reads: centre, conic, opacity, tile box"""
    n = len(xy)
    rec = np.zeros((n, REC), np.float32)
    rec[:, 0:2], rec[:, 2:5], rec[:, 5] = xy, conic, op
    x0, y0, x1, y1 = (np.asarray(v, np.int64) for v in box)
    rec[:, 10] = (x0 | (y0 << 16)).astype(np.uint32).view(np.float32)
    rec[:, 11] = (x1 | (y1 << 16)).astype(np.uint32).view(np.float32)
    return rec


def circle_box(xy, radius, W, H, pad=0.0):
    """tile box of the circle of `radius` pixels (+ pad) around xy: (int)(c / 16 - r / 16), (int)(c / 16 + r / 16 + 1),
    clamped to the tile grid — the upstream rule in float64"""
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    r = (np.asarray(radius, np.float64) + pad) / TILE
    c = np.asarray(xy, np.float64) / TILE
    x0, x1 = np.trunc(c[:, 0] - r), np.trunc(c[:, 0] + r + 1.0)
    y0, y1 = np.trunc(c[:, 1] - r), np.trunc(c[:, 1] + r + 1.0)
    x0, x1 = np.clip(x0, 0, tx).astype(np.int64), np.clip(x1, 0, tx).astype(np.int64)
    y0, y1 = np.clip(y0, 0, ty).astype(np.int64), np.clip(y1, 0, ty).astype(np.int64)
    empty = (x1 <= x0) | (y1 <= y0)
    for v in (x0, y0, x1, y1):
        v[empty] = 0
    return x0, y0, x1, y1


def box_pairs(rec):
    """every (record, tile) pair of the boxes, records in order, tiles in (y, x) order: (off [n + 1], ri, tx, ty)"""
    x0, y0, x1, y1 = boxes_of(rec)
    w, h = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    area = w * h
    off = np.concatenate([[0], np.cumsum(area)])
    ri = np.repeat(np.arange(len(rec)), area)
    local = np.arange(off[-1]) - off[ri]
    wr = np.maximum(w[ri], 1)
    return off, ri, x0[ri] + local % wr, y0[ri] + local // wr


# ---- the ellipse test -------------------------------------------------------------------------------------------------
def _f64(rec, ri):
    r = rec[ri].astype(np.float64)
    return r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]


def sigma(a, b, c, dx, dy):
    return 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy


def well_conditioned(rec):
    r = rec.astype(np.float64)
    a, b, c = r[:, 2], r[:, 3], r[:, 4]
    return (a > 0) & (c > 0) & (a * c - b * b >= 1e-3 * a * c)


def rect_min_sigma(a, b, c, u0, u1, v0, v1):
    """minimum of sigma over the rectangle [u0, u1] x [v0, v1] of offsets from the centre, for a positive definite conic:
    0 when the rectangle holds the centre, else the smallest of the four edge minima (clamped 1-D quadratics)"""
    def edge_u(u):                     # u fixed, v free
        v = np.clip(-b * u / c, v0, v1)
        return sigma(a, b, c, u, v)

    def edge_v(v):
        u = np.clip(-b * v / a, u0, u1)
        return sigma(a, b, c, u, v)
    m = np.minimum(np.minimum(edge_u(u0), edge_u(u1)), np.minimum(edge_v(v0), edge_v(v1)))
    inside = (u0 <= 0) & (u1 >= 0) & (v0 <= 0) & (v1 >= 0)
    return np.where(inside, 0.0, m)


def _row_times(ty, H, t_min, t_max, t_ro):
    """time interval over the pixel rows of tile row ty that lie inside the image"""
    ya, yb = ty * TILE + 0.5, np.minimum(ty * TILE + TILE - 0.5, H - 0.5)
    ta, tb = (ya / H - 0.5) * t_ro, (yb / H - 0.5) * t_ro
    return min(t_min, t_max) + np.minimum(ta, tb), max(t_min, t_max) + np.maximum(ta, tb)


def _tile_rect(gx, gy, tx, ty, W, H, clip_cols):
    u0, u1 = tx * TILE + 0.5 - gx, tx * TILE + TILE - 0.5 - gx
    if clip_cols:
        u1 = np.minimum(tx * TILE + TILE - 0.5, W - 0.5) - gx
    v0, v1 = ty * TILE + 0.5 - gy, np.minimum(ty * TILE + TILE - 0.5, H - 0.5) - gy
    return u0, u1, v0, v1


def _sweep_box(ty, H, vx, vy, sweep):
    t_lo, t_hi = _row_times(ty, H, sweep["t_min"], sweep["t_max"], sweep["t_ro"])
    ox0, ox1 = np.minimum(t_lo * vx, t_hi * vx), np.maximum(t_lo * vx, t_hi * vx)
    oy0, oy1 = np.minimum(t_lo * vy, t_hi * vy), np.maximum(t_lo * vy, t_hi * vy)
    slack = 1e-3 + 1e-5 * (np.abs(t_lo) + np.abs(t_hi)) * (np.abs(vx) + np.abs(vy))
    return ox0, ox1, oy0, oy1, slack


def loose_hits(rec, ri, tx, ty, W, H, sweep=None):
    """vectorised loose_hit of the pairs (ri, tx, ty); meaningful where well_conditioned(rec)[ri].
    sweep: None or dict(pix_vel [n, 2], t_min, t_max, t_ro)"""
    gx, gy, a, b, c, o = _f64(rec, ri)
    with np.errstate(all="ignore"):
        tau = np.log(255.0 * o)
        det = a * c - b * b
        uext = np.sqrt(np.maximum(2.0 * np.maximum(tau, 0) * c / det, 0.0))
        grow = 4e-3 + 4e-6 * (np.abs(gx) + uext)
        u0, u1, v0, v1 = _tile_rect(gx, gy, tx, ty, W, H, clip_cols=False)
        u0, u1, v0, v1 = u0 - grow, u1 + grow, v0 - grow, v1 + grow
        if sweep is not None:
            pv = sweep["pix_vel"].astype(np.float64)[ri]
            ox0, ox1, oy0, oy1, slack = _sweep_box(ty, H, pv[:, 0], pv[:, 1], sweep)
            u0, u1, v0, v1 = u0 - ox1 - 2 * slack, u1 - ox0 + 2 * slack, v0 - oy1 - 2 * slack, v1 - oy0 + 2 * slack
        m = rect_min_sigma(a, b, c, u0, u1, v0, v1)
        return (tau >= 0) & (m <= 1.003 * tau + 3e-3)


def _strict_static_rows(rec, ri, tx, ty, W, H):
    """exact: per pixel row of the tile, sigma is a convex quadratic in dx (a > 0), so its smallest value over the row's
    pixel centres is at one of the two centres next to the continuous minimiser"""
    gx, gy, a, b, c, o = _f64(rec, ri)
    best = np.full(len(ri), np.inf)
    xlo, xhi = tx * TILE, np.minimum(tx * TILE + TILE, W) - 1            # pixel columns inside the image
    with np.errstate(all="ignore"):
        for k in range(TILE):
            py = ty * TILE + k
            dy = py + 0.5 - gy
            xs = gx - b * dy / a - 0.5                                      # continuous minimiser, as a pixel index
            for cand in (np.floor(xs), np.floor(xs) + 1.0):
                px = np.clip(cand, xlo, xhi)
                s = sigma(a, b, c, px + 0.5 - gx, dy)
                best = np.where((py < H) & (xhi >= xlo), np.minimum(best, s), best)
        return o * np.exp(-best) >= ALPHA_MIN


def _strict_pixels(rec, ri, tx, ty, W, H, sweep=None, chunk=20000):
    """brute force over all 256 pixel centres of each tile (the definition itself); sweep as in loose_hits"""
    out = np.zeros(len(ri), bool)
    k = np.arange(TILE)
    for s0 in range(0, len(ri), chunk):
        sl = slice(s0, s0 + chunk)
        gx, gy, a, b, c, o = (v[:, None, None] for v in _f64(rec, ri[sl]))
        px = (tx[sl, None, None] * TILE + k[None, None, :]).astype(np.float64)
        py = (ty[sl, None, None] * TILE + k[None, :, None]).astype(np.float64)
        inside = (px < W) & (py < H)
        dx, dy = px + 0.5 - gx, py + 0.5 - gy
        with np.errstate(all="ignore"):
            if sweep is None:
                s = sigma(a, b, c, dx, dy)
            else:
                pv = sweep["pix_vel"].astype(np.float64)[ri[sl]]
                vx, vy = pv[:, 0, None, None], pv[:, 1, None, None]
                tr = ((py + 0.5) / H - 0.5) * sweep["t_ro"]
                lo, hi = min(sweep["t_min"], sweep["t_max"]) + tr, max(sweep["t_min"], sweep["t_max"]) + tr
                q2 = sigma(a, b, c, vx, vy)                               # sigma(d - t v) = sigma(d) - t q1 + t^2 q2
                q1 = a * dx * vx + c * dy * vy + b * (dx * vy + dy * vx)
                t = np.clip(np.where(q2 > 0, q1 / (2 * np.where(q2 > 0, q2, 1.0)), lo), lo, hi)
                s = np.minimum(np.minimum(sigma(a, b, c, dx - t * vx, dy - t * vy), sigma(a, b, c, dx - lo * vx, dy - lo * vy)),
                               sigma(a, b, c, dx - hi * vx, dy - hi * vy))
            al = np.where(inside, o * np.exp(-s), 0.0)
        out[sl] = (al >= ALPHA_MIN).any(axis=(1, 2))
    return out


def strict_candidates(rec, ri, tx, ty, W, H, sweep=None):
    """a superset of the strict pairs that is cheap to compute: for a positive definite conic (float64) the minimum of
    sigma over the tile's continuous pixel-centre rectangle (widened by the swept offsets' box) bounds every pixel's
    sigma from below; pairs where it exceeds ln(255 o) (1 + 1e-9) cannot be strict.  Other conics are all candidates."""
    gx, gy, a, b, c, o = _f64(rec, ri)
    with np.errstate(all="ignore"):
        tau = np.log(255.0 * o)
        pd = (a > 0) & (c > 0) & (a * c - b * b > 0)
        u0, u1, v0, v1 = _tile_rect(gx, gy, tx, ty, W, H, clip_cols=True)
        if sweep is not None:
            pv = sweep["pix_vel"].astype(np.float64)[ri]
            ox0, ox1, oy0, oy1, _ = _sweep_box(ty, H, pv[:, 0], pv[:, 1], sweep)
            u0, u1, v0, v1 = u0 - ox1, u1 - ox0, v0 - oy1, v1 - oy0
        m = rect_min_sigma(a, b, c, u0, u1, v0, v1)
        return (o > 0) & ~(tau < 0) & (~pd | ~(m > tau * (1 + 1e-9) + 1e-12))


def strict_hits(rec, ri, tx, ty, W, H, sweep=None, only=None):
    """vectorised strict_hit of the pairs; `only` (bool mask) restricts the evaluation (False elsewhere)"""
    cand = strict_candidates(rec, ri, tx, ty, W, H, sweep)
    if only is not None:
        cand &= only
    out = np.zeros(len(ri), bool)
    idx = np.nonzero(cand)[0]
    if idx.size:
        if sweep is None:
            out[idx] = _strict_static_rows(rec, ri[idx], tx[idx], ty[idx], W, H)
        else:
            out[idx] = _strict_pixels(rec, ri[idx], tx[idx], ty[idx], W, H, sweep)
    return out


def strict_hit(rec, tx, ty, W, H, sweep=None):
    """one pair, by the definition (every pixel of the tile); rec: one record"""
    r = np.asarray(rec, np.float32).reshape(1, -1)
    sw = None if sweep is None else dict(sweep, pix_vel=np.asarray(sweep["pix_vel"], np.float32).reshape(1, 2))
    return bool(_strict_pixels(r, np.zeros(1, np.int64), np.array([tx]), np.array([ty]), W, H, sw)[0])


def loose_hit(rec, tx, ty, W, H, sweep=None):
    r = np.asarray(rec, np.float32).reshape(1, -1)
    sw = None if sweep is None else dict(sweep, pix_vel=np.asarray(sweep["pix_vel"], np.float32).reshape(1, 2))
    return bool(loose_hits(r, np.zeros(1, np.int64), np.array([tx]), np.array([ty]), W, H, sw)[0])


# ---- integer contracts ------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def slice_plan(P, N, K, cum, total, base, n_live=None, grand=None):
    """cum: the exclusive prefix of the counts over all P*N ranks (uint32, modulo 2^32); total: the grand total.
    -> bounds [P*K], rels [P*K], seg_totals [P], tail [P + 1]"""
    cum = np.asarray(cum, np.uint64)
    bounds, rels = np.zeros(P * K, np.int64), np.zeros(P * K, np.int64)
    seg, tail = np.zeros(P, np.int64), np.zeros(P + 1, np.int64)
    for p in range(P):
        c = cum[p * N:(p + 1) * N].astype(np.int64)
        c0 = int(c[0])
        M = N if n_live is None else min(N, int(n_live[p]))
        seg_end = int(cum[(p + 1) * N]) if p + 1 < P else int(total)
        rel = (c[:M] - c0) & M32
        for k in range(K):
            tgt = int(base) << k
            hit = np.nonzero(rel >= tgt)[0]
            # the kernel's binary search assumes rel is non-decreasing over the live ranks
            lo = int(hit[0]) if hit.size else M
            bounds[p * K + k] = lo
            rels[p * K + k] = ((int(c[lo]) if lo < M else seg_end) - c0) & M32
        seg[p] = (seg_end - c0) & M32
        tail[p] = M
    tail[P] = int(total if grand is None else grand) & M32
    return bounds, rels, seg, tail


def open_sat(done, P, tiles_x, tiles_y):
    """done [P, tiles_y, tiles_x] uint8 -> (sat [P, tiles_y + 1, tiles_x + 1] int, open_bits [P, tiles_y, W64] uint64)"""
    opn = (np.asarray(done).reshape(P, tiles_y, tiles_x) == 0)
    sat = np.zeros((P, tiles_y + 1, tiles_x + 1), np.int64)
    sat[:, 1:, 1:] = opn.cumsum(1).cumsum(2)
    w64 = (tiles_x + 63) // 64
    bits = np.zeros((P, tiles_y, w64), np.uint64)
    for x in range(tiles_x):
        bits[:, :, x >> 6] |= opn[:, :, x].astype(np.uint64) << np.uint64(x & 63)
    return sat, bits


def box_counts(rec, gi, N, done, tiles_x, tiles_y):
    """open tiles of the box of every slice Gaussian gi[j] (done None: the box area)"""
    x0, y0, x1, y1 = (v[gi] for v in boxes_of(rec))
    area = np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)
    if done is None:
        return area
    P = len(rec) // N
    sat, _ = open_sat(done, P, tiles_x, tiles_y)
    p = gi // N
    return np.where(area > 0, sat[p, y1, x1] - sat[p, y0, x1] - sat[p, y1, x0] + sat[p, y0, x0], 0)


def mask_layout(rec, sorted_gi, ranks):
    """slice Gaussian j sits at depth rank ranks[j]; cum_rank = exclusive prefix of the BOX areas in rank order;
    mask_off[j] = (cum_rank[rank] >> 6) + j, and Gaussian j owns ceil(area / 64) words from there"""
    x0, y0, x1, y1 = (v[sorted_gi] for v in boxes_of(rec))
    area = np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)
    cum_rank = (np.concatenate([[0], np.cumsum(area)[:-1]]) & M32).astype(np.int64)
    j = np.arange(len(ranks))
    return cum_rank, (cum_rank[ranks] >> 6) + j, (area[ranks] + 63) >> 6


def unpack_mask(words, moff, area):
    """bits 0 .. area-1 of the little-endian bit string starting at word moff"""
    nw = (area + 63) >> 6
    w = np.asarray(words[moff:moff + nw], np.uint64)
    bits = ((w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
    return bits[:area], bits[area:]


def expand(bits_of, gi, rec, N, tiles_x, T):
    """emission of the slice: for Gaussian j in order, its set bits in (y, x) order: key = p T + ty tiles_x + tx,
    value = gi = p N + g.  bits_of[j]: bool [area] in box order.  -> keys, vals, per-Gaussian counts"""
    x0, y0, x1, y1 = boxes_of(rec)
    keys, vals, cnt = [], [], []
    for j, g in enumerate(gi):
        b = np.nonzero(bits_of[j])[0]
        w = max(int(x1[g] - x0[g]), 1)
        keys.append((g // N) * T + (y0[g] + b // w) * tiles_x + x0[g] + b % w)
        vals.append(np.full(b.size, g))
        cnt.append(b.size)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(keys).astype(np.int64), cat(vals).astype(np.int64), np.asarray(cnt, np.int64)


def tile_hot(keys, vals, rec, n_tiles):
    hot = np.zeros(n_tiles, np.uint8)
    sel = rec[vals, 5] > ALPHA_MAX
    hot[keys[sel]] = 1
    return hot


def segmented_exclusive_scan(x, seg_len, seg_counts):
    """one running sum over the whole array in which only the first seg_counts[s] elements of every segment count;
    defined at the live ranks and at every segment's first rank.  -> (out, defined mask, total)"""
    x = np.asarray(x, np.int64)
    n = len(x)
    live = (np.arange(n) % seg_len) < np.repeat(np.asarray(seg_counts, np.int64), seg_len)
    v = np.where(live, x, 0)
    out = (np.concatenate([[0], np.cumsum(v)[:-1]])) & M32
    return out, live | (np.arange(n) % seg_len == 0), int(v.sum()) & M32


def gather_counts(sorted_gi, num_tiles_hit):
    return np.asarray(num_tiles_hit, np.int64)[np.asarray(sorted_gi, np.int64)] & M32


def depth_keys64(depth_keys, N):
    dk = np.asarray(depth_keys, np.uint64)
    return ((np.arange(len(dk), dtype=np.uint64) // np.uint64(N)) << np.uint64(32)) | dk
