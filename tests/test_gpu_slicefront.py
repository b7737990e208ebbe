"""The slice front end of csrc/binning.hip kernel by kernel at the C ABI, against tests/slicefront_reference.py (numpy,
float64) and the host build of csrc/tilecull_math.h: gs_tile_open_sat, gs_slice_counts, gs_slice_counts_exact(_swept),
gs_emit_open_intersects, gs_emit_intersects, gs_slice_plan(_select), gs_exclusive_scan_segments_u32, gs_gather_counts,
gs_make_depth_keys64.  No image is rendered: records come from gs_pack_records over hand-made splats, the test supplies
sorted_gi and so chooses which Gaussians share a wave.

The count kernel picks its code path from a box's size and its company in the wave; the constants are restated here and
every case asserts BY CONSTRUCTION (from the boxes it reads back) that its wave meets the condition of the path it names."""
import ctypes

import numpy as np
import pytest
import torch

import slicefront_reference as R
from test_slicefront_host import NEEDLES, host_bits, load_host

pytestmark = pytest.mark.gpu

# csrc/binning.hip
K_SOLO, K_SOLO_MAX, K_SOLO_MANY, K_MID_MAX, K_MASK_WORDS = 12, 64, 4, 256, 512
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 1024
G1, G2, G3 = (2048, 200), (4096, 2064), (40, 24)
P_SUB = 2


def tiles(W, H):
    return (W + 15) // 16, (H + 15) // 16


def hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def conic_of(s1, s2, th):
    cs, sn, l1, l2 = np.cos(th), np.sin(th), s1 * s1, s2 * s2
    cxx, cxy, cyy = cs * cs * l1 + sn * sn * l2, cs * sn * (l1 - l2), sn * sn * l1 + cs * cs * l2
    det = l1 * l2
    return cyy / det, -cxy / det, cxx / det


class Scene:
    """P_SUB sub-poses of N splats; sub-pose 1 holds the same splats shifted by one tile and in another depth order"""

    def __init__(self, gs, dev, geom, splats, seed):
        from gsdeblur_amd import _lib
        from gsdeblur_amd.ops import _ptr, _stream
        self.L, self._ptr, self._stream, self.check, self.dev = _lib.load(), _ptr, _stream, _lib.check, dev
        self.W, self.H = geom
        self.tx, self.ty = tiles(*geom)
        self.T = self.tx * self.ty
        rng = np.random.default_rng(seed)
        n = len(splats)
        self.N = n
        xy = np.zeros((P_SUB * n, 2), np.float32)
        conic = np.zeros((P_SUB * n, 3), np.float32)
        op = np.zeros(P_SUB * n, np.float32)
        rad = np.zeros(P_SUB * n, np.int32)
        for i, (cx, cy, r, kind) in enumerate(splats):
            aniso = (1.0, 3.0, 10.0)[i % 3]
            s1 = max(r / 3.0, 0.5)
            a, b, c = conic_of(s1, max(s1 / aniso, 0.3), rng.random() * np.pi)
            o = (0.05, 0.5, 0.9995, 1.02 / 255, 0.2)[i % 5]
            if kind == "faint":
                o = (0.9 / 255, 0.0)[i % 2]
            if kind == "degenerate":
                a, b, c = 0.01, 0.01, 0.01
            if isinstance(kind, tuple):                      # conic and opacity given; sub-pose 0 at exactly (cx, cy)
                a, b, c, o = kind
            for p in range(P_SUB):
                k = p * n + i
                jitter = (0.0, 0.0) if isinstance(kind, tuple) and p == 0 else (rng.random() - 0.5, rng.random() - 0.5)
                xy[k] = (cx + 16 * p + jitter[0], cy + jitter[1])
                conic[k], op[k], rad[k] = (a, b, c), o, r
        t = lambda a: torch.from_numpy(a).to(dev)
        self.rec_t = torch.zeros(P_SUB * n, 16, dtype=torch.float32, device=dev)
        dk = torch.zeros(P_SUB * n, dtype=torch.int32, device=dev)
        self.ntiles_t = torch.zeros(P_SUB * n, dtype=torch.int32, device=dev)
        col = torch.from_numpy(np.random.default_rng(seed + 1000).random((P_SUB * n, 3)).astype(np.float32)).to(dev)
        dep = torch.ones(P_SUB * n, dtype=torch.float32, device=dev)
        xy_t, rad_t, conic_t, op_t = t(xy), t(rad), t(conic), t(op)
        self.check(self.L.gs_pack_records(P_SUB * n, _ptr(xy_t), _ptr(dep), _ptr(rad_t), _ptr(conic_t), _ptr(col),
                                          _ptr(op_t), self.H, self.W, _ptr(self.rec_t), _ptr(dk), _ptr(self.ntiles_t),
                                          _stream()), "pack")
        self.rec = self.rec_t.cpu().numpy()
        self.x0, self.y0, self.x1, self.y1 = R.boxes_of(self.rec)
        self.area = (self.x1 - self.x0) * (self.y1 - self.y0)
        assert np.array_equal(self.area, self.ntiles_t.cpu().numpy())
        self.pix_vel = ((rng.random((n, 2)) - 0.5) * 600).astype(np.float32)
        # depth orders: "designed" keeps the splats of a wave together (sub-pose 1 rotated by 7 inside each wave of 64),
        # "mixed" strides through them so that every splat gets other company
        w = np.arange(n)
        rot = (w // 64) * 64 + ((w % 64) + 7) % np.minimum(64, n - (w // 64) * 64)
        self.orders = {"designed": np.concatenate([w, n + rot]),
                       "mixed": np.concatenate([(w * 37) % n if np.gcd(37, n) == 1 else w[::-1], n + w[::-1]])}
        self._ref = {}

    # ---- reference decisions per (record, tile), shared by every variant -------------------------------------------
    def ref(self, sweep=None):
        key = None if sweep is None else (sweep["t_min"], sweep["t_max"], sweep["t_ro"])
        if key not in self._ref:
            sw = None if sweep is None else dict(sweep, pix_vel=np.tile(self.pix_vel, (P_SUB, 1)))
            off, ri, tx, ty = R.box_pairs(self.rec)
            strict = R.strict_hits(self.rec, ri, tx, ty, self.W, self.H, sw)
            loose = R.loose_hits(self.rec, ri, tx, ty, self.W, self.H, sw) | ~R.well_conditioned(self.rec)[ri]
            host = host_bits(load_host(), self.rec, self.W, self.H, sw, 0)
            self._ref[key] = dict(off=off, ri=ri, tx=tx, ty=ty, strict=strict, loose=loose, host=host)
        return self._ref[key]

    def slice_of(self, order, skip):
        """the slice = ranks [p N + skip, (p + 1) N) of every sub-pose -> (sorted_gi, begin, prefix, ranks, gi)"""
        n = self.N
        sgi = self.orders[order]
        begin = np.array([p * n + skip for p in range(P_SUB)], np.int32)
        prefix = np.array([p * (n - skip) for p in range(P_SUB + 1)], np.int32)
        ranks = np.concatenate([np.arange(p * n + skip, (p + 1) * n) for p in range(P_SUB)])
        return sgi, begin, prefix, ranks, sgi[ranks]

    def open_tables(self, done):
        """gs_tile_open_sat, checked against numpy"""
        d_t = torch.from_numpy(done.reshape(-1)).to(self.dev)
        nsat, w64 = P_SUB * (self.ty + 1) * (self.tx + 1), (self.tx + 63) // 64
        sat = torch.full((GUARD + nsat + GUARD,), POISON32, dtype=torch.int32, device=self.dev)
        ob = torch.full((GUARD + P_SUB * self.ty * w64 + GUARD,), POISON64, dtype=torch.int64, device=self.dev)
        self.check(self.L.gs_tile_open_sat(P_SUB, self.H, self.W, self._ptr(d_t), self._ptr(sat[GUARD:]),
                                           self._ptr(ob[GUARD:]), None, self._stream()), "sat")
        want_sat, want_bits = R.open_sat(done, P_SUB, self.tx, self.ty)
        s, o = sat.cpu().numpy(), ob.cpu().numpy().view(np.uint64)
        assert np.array_equal(s[GUARD:-GUARD], want_sat.reshape(-1))
        assert np.array_equal(o[GUARD:-GUARD], want_bits.reshape(-1))
        assert (s[:GUARD] == POISON32).all() and (s[-GUARD:] == POISON32).all()
        assert (o[:GUARD] == POISON64).all() and (o[-GUARD:] == POISON64).all()
        return d_t, sat[GUARD:GUARD + nsat], ob[GUARD:GUARD + P_SUB * self.ty * w64]

    def counts_exact(self, order="designed", skip=0, done=None, wpg=0, masks=True, gate=None, sweep=None):
        """-> dict(counts, slice_gi, gi, bits (list of bool [area] per slice Gaussian, None without masks), words, moff)"""
        sgi, begin, prefix, ranks, gi = self.slice_of(order, skip)
        ns = len(gi)
        sgi_t = torch.from_numpy(sgi.astype(np.int32)).to(self.dev)
        cum_rank, want_moff, nw = R.mask_layout(self.rec, sgi, ranks)
        n_words = int((want_moff + nw).max())
        buf = lambda n, dt, poison: torch.full((GUARD + n + GUARD,), poison, dtype=dt, device=self.dev)
        cnt, sg, mo = buf(ns, torch.int32, POISON32), buf(ns, torch.int32, POISON32), buf(ns, torch.int32, POISON32)
        mw = buf(n_words, torch.int64, POISON64)
        cr_t = torch.from_numpy(cum_rank.astype(np.uint32).view(np.int32)).to(self.dev)
        d_t = sat = ob = None
        if done is not None:
            d_t, sat, ob = self.open_tables(done)
        g_t = None if gate is None else torch.tensor([gate], dtype=torch.int32, device=self.dev)
        pm = self._ptr
        common = (ns, P_SUB, self.N, hp(begin), hp(prefix), pm(sgi_t), pm(self.rec_t), pm(sat), pm(d_t), self.H, self.W,
                  pm(sg[GUARD:]), pm(cnt[GUARD:]), wpg, pm(cr_t) if masks else None, pm(mw[GUARD:]) if masks else None,
                  pm(mo[GUARD:]) if masks else None, pm(ob))
        if sweep is None:
            self.check(self.L.gs_slice_counts_exact(*common, pm(g_t), self._stream()), "counts_exact")
        else:
            pv = torch.from_numpy(self.pix_vel).to(self.dev)
            self.check(self.L.gs_slice_counts_exact_swept(*common, pm(pv), sweep["t_min"], sweep["t_max"], sweep["t_ro"],
                                                          self._stream()), "counts_exact_swept")
        cnt_h, sg_h, mo_h = cnt.cpu().numpy(), sg.cpu().numpy(), mo.cpu().numpy()
        mw_h = mw.cpu().numpy().view(np.uint64)
        for a, poison in ((cnt_h, POISON32), (sg_h, POISON32), (mo_h, POISON32), (mw_h, POISON64)):
            assert (a[:GUARD] == poison).all() and (a[-GUARD:] == poison).all(), "guard region written"
        out = dict(gi=gi, counts=cnt_h[GUARD:-GUARD].astype(np.int64), ranks=ranks, sgi=sgi, begin=begin, prefix=prefix,
                   slice_gi_t=sg[GUARD:GUARD + ns], counts_t=cnt[GUARD:GUARD + ns], words_t=mw[GUARD:GUARD + n_words],
                   moff_t=mo[GUARD:GUARD + ns], bits=None, done_t=d_t, sat=sat)
        if gate == 0:
            assert (out["counts"] == 0).all() and (mw_h == POISON64).all() and (mo_h == POISON32).all()
            return out
        assert np.array_equal(sg_h[GUARD:-GUARD], gi)
        if not masks:
            assert (mw_h == POISON64).all() and (mo_h == POISON32).all()
            return out
        assert np.array_equal(mo_h[GUARD:-GUARD], want_moff)
        words = mw_h[GUARD:-GUARD]
        owned = np.zeros(n_words, bool)
        bits = []
        for j in range(ns):
            a = int(self.area[gi[j]])
            owned[want_moff[j]:want_moff[j] + nw[j]] = True
            w = words[want_moff[j]:want_moff[j] + nw[j]]
            if a == 0 or (out["counts"][j] == 0 and (w == POISON64).all()):    # rejected before the walk: words untouched
                assert out["counts"][j] == 0
                bits.append(np.zeros(a, bool))
                continue
            inside, beyond = R.unpack_mask(words, int(want_moff[j]), a)
            assert not beyond.any(), ("bit beyond the box", j)
            assert int(inside.sum()) == out["counts"][j], ("count != popcount", j)
            bits.append(inside)
        assert (words[~owned] == POISON64).all(), "a word between two Gaussians' ranges was written"
        out["bits"] = bits
        return out

    def check_bits(self, res, done, sweep=None):
        """the decisions of one run against the references -> (kept, strict) pair counts over its open tiles"""
        ref = self.ref(sweep)
        kept = nstrict = 0
        for j, g in enumerate(res["gi"]):
            sl = slice(ref["off"][g], ref["off"][g + 1])
            opn = np.ones(sl.stop - sl.start, bool) if done is None else \
                done[g // self.N, ref["ty"][sl], ref["tx"][sl]] == 0
            b = res["bits"][j]
            assert not (b & ~opn).any(), ("bit on a closed tile", j)
            assert not (ref["strict"][sl] & opn & ~b).any(), ("strict pair culled", j, int(g))
            assert not (b & ~ref["loose"][sl]).any(), ("kept pair outside loose_hit", j, int(g))
            kept += int(b.sum())
            nstrict += int((ref["strict"][sl] & opn).sum())
        return kept, nstrict

    def bits_by_record(self, res):
        return {int(g): res["bits"][j] for j, g in enumerate(res["gi"])}

    def done_states(self, seed):
        rng = np.random.default_rng(seed)
        shape = (P_SUB, self.ty, self.tx)
        one = np.ones(shape, np.uint8)
        one[0, self.ty // 2, self.tx // 2] = 0
        one[1, self.ty - 1, self.tx - 1] = 0
        sub = np.zeros(shape, np.uint8)
        sub[1] = 1
        return {"all open": np.zeros(shape, np.uint8), "random half": (rng.random(shape) < 0.5).astype(np.uint8),
                "all closed but one tile": one, "one sub-pose closed": sub}


# ---- the scenes: one wave of 64 per targeted path ------------------------------------------------------------------------
def filler(k, geom):
    """area <= 12: boxes of 1 .. 3 x 1 .. 3 tiles spread over the image"""
    W, H = geom
    return ((k * 131) % W + 0.5, (k * 37) % H + 0.5, (4, 8, 16, 6)[k % 4], "plain")


def wave(geom, special, n=64):
    """n splats: the special ones at fixed, spread slots, fillers elsewhere, two faint and one degenerate splat among them"""
    out = [filler(k, geom) for k in range(n)]
    out[5] = out[5][:3] + ("faint",)
    out[6] = out[6][:3] + ("faint",)
    out[9] = out[9][:3] + ("degenerate",)
    slots = [3, 17, 18, 40, 41, 42, 55, 63, 11, 29]
    for s, sp in zip(slots, special):
        out[s] = sp + ("plain",) if len(sp) == 3 else sp
    return out


def spec_for(path):
    """-> (geometry, splats, predicate on the special boxes (area, w, h, x0), how many specials the wave must hold)"""
    if path == "solo: area <= 12":
        return G1, wave(G1, []), None, 0
    if path == "solo limit raised: >= 4 boxes of 13..64 tiles in the wave":
        sp = [(300.0, 100.0, 32), (700.0, 90.0, 48), (1100.0, 110.0, 56), (1500.0, 100.0, 24), (1900.0, 100.0, 40)]
        return G1, wave(G1, sp), lambda a, w, h, x0: K_SOLO < a <= K_SOLO_MAX, 5
    if path == "wave-cooperative: 2 boxes of 13..64 tiles in the wave":
        sp = [(300.0, 100.0, 32), (1500.0, 100.0, 56)]
        return G1, wave(G1, sp), lambda a, w, h, x0: K_SOLO < a <= K_SOLO_MAX, 2
    if path == "mid: >= 4 boxes of 65..256 tiles, w <= 64, words crossed":
        sp = [(300.0, 104.0, 64), (700.0, 104.0, 96), (1100.0, 104.0, 120), (1500.0, 104.0, 80), (1900.0, 104.0, 72)]
        return G1, wave(G1, sp), lambda a, w, h, x0: K_SOLO_MAX < a <= K_MID_MAX and w <= 64 and (w * h) % 64 != 0, 5
    if path == "wave-cooperative: 2 boxes of 65..256 tiles, w <= 64":
        sp = [(300.0, 104.0, 64), (1500.0, 104.0, 120)]
        return G1, wave(G1, sp), lambda a, w, h, x0: K_SOLO_MAX < a <= K_MID_MAX and w <= 64, 2
    if path == "w > 64: 64-column chunks":
        sp = [(1024.0, 100.0, 700), (600.0, 60.0, 2000), (1500.0, 150.0, 560)]
        return G1, wave(G1, sp), lambda a, w, h, x0: w > 64, 3
    if path == "x0 & 63 != 0 across a 64-tile boundary, prefetched words (lane-private)":
        sp = [(1024.0, 100.0, 56), (1030.0, 60.0, 96), (1000.0, 120.0, 120), (1040.0, 100.0, 48), (1016.0, 90.0, 88)]
        return G1, wave(G1, sp), lambda a, w, h, x0: a > K_SOLO and w <= 64 and a <= K_MID_MAX and x0 & 63 and \
            (x0 >> 6) != ((x0 + w - 1) >> 6), 5
    if path == "x0 & 63 != 0 across a 64-tile boundary, row_window (wave-cooperative)":
        sp = [(1024.0, 100.0, 56), (1000.0, 120.0, 300)]
        return G1, wave(G1, sp), lambda a, w, h, x0: a > K_SOLO and x0 & 63 and (x0 >> 6) != ((x0 + w - 1) >> 6), 2
    if path == "more than 64 box rows":
        sp = [(2000.0, 1000.0, 560), (1000.0, 1200.0, 900)]
        return G2, wave(G2, sp), lambda a, w, h, x0: h > 64 and (a + 63) // 64 <= K_MASK_WORDS, 2
    if path == "area > 32768: beyond the LDS bit string":
        sp = [(2048.0, 1032.0, 5000)]
        return G2, wave(G2, sp), lambda a, w, h, x0: (a + 63) // 64 > K_MASK_WORDS, 1
    if path == "needles: determinant inside its float32 rounding error":
        sp = [(x, y, 6000, (a, b, c, o)) for x, y, a, b, c, o in NEEDLES]
        return G1, wave(G1, sp), lambda a, w, h, x0: a == 128 * 13, len(NEEDLES)
    if path == "partial tiles both ways":
        sp = [(20.0, 12.0, 30), (5.0, 20.0, 12), (38.0, 2.0, 20)]
        return G3, wave(G3, sp, n=24), None, 0
    raise KeyError(path)


PATHS = ["solo: area <= 12", "solo limit raised: >= 4 boxes of 13..64 tiles in the wave",
         "wave-cooperative: 2 boxes of 13..64 tiles in the wave", "mid: >= 4 boxes of 65..256 tiles, w <= 64, words crossed",
         "wave-cooperative: 2 boxes of 65..256 tiles, w <= 64", "w > 64: 64-column chunks",
         "x0 & 63 != 0 across a 64-tile boundary, prefetched words (lane-private)",
         "x0 & 63 != 0 across a 64-tile boundary, row_window (wave-cooperative)", "more than 64 box rows",
         "area > 32768: beyond the LDS bit string", "partial tiles both ways",
         "needles: determinant inside its float32 rounding error"]
SWEPT_PATHS = [p for p in PATHS if spec_for(p)[0] != G2]
_scenes = {}


def scene_for(gs, dev, path):
    if path not in _scenes:
        geom, splats, pred, n_special = spec_for(path)
        S = Scene(gs, dev, geom, splats, seed=PATHS.index(path))
        # by construction: wave 0 of the designed order (sub-pose 0, ranks 0..63) holds exactly the boxes the path needs
        idx = np.arange(min(64, S.N))
        a, w, h, x0 = S.area[idx], (S.x1 - S.x0)[idx], (S.y1 - S.y0)[idx], S.x0[idx]
        big = a > K_SOLO
        if pred is None:
            assert not big.any() or geom == G3
        else:
            hit = np.array([bool(pred(int(a[i]), int(w[i]), int(h[i]), int(x0[i]))) for i in idx])
            assert int(hit.sum()) == n_special and int(big.sum()) == n_special, (path, a[big], w[big], h[big], x0[big])
        S.special = np.nonzero(big)[0]
        _scenes[path] = S
    return _scenes[path]


# ---- gs_slice_counts_exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_exact_counts_and_hit_masks(gs, dev, path):
    """counts == popcount of the mask words; mask layout; no bit outside box and open; every open strict pair kept; every
    kept pair of a well-conditioned conic a loose hit; identical decisions across wave_per_gaussian, masks, tile_done
    states, slice offsets and company in the wave; guard regions; the host build's bits"""
    S = scene_for(gs, dev, path)
    ref = S.ref()
    base = S.counts_exact()
    kept, nstrict = S.check_bits(base, None)
    by_rec = S.bits_by_record(base)
    assert kept > 0 and nstrict > 0
    total = int(sum(S.area[g] for g in base["gi"]))
    assert kept < total or S.W == 40, "the cull culls"
    # GPU against the host build: they may differ through __logf against logf only
    differ = 0
    for g, b in by_rec.items():
        sl = slice(ref["off"][g], ref["off"][g + 1])
        d = b != ref["host"][sl]
        differ += int(d.sum())
        assert not (d & ref["strict"][sl]).any() and (ref["loose"][sl] | ~d).all()
    print(f"[{path}] pairs {total} kept {kept} strict {nstrict} kept/strict {kept / nstrict:.4f} GPU != host build: {differ}")
    # every other variant takes the same decision for every (record, tile)
    for order, skip, wpg in (("designed", 0, 1), ("mixed", 0, 0), ("designed", 5, 0), ("mixed", 3, 1)):
        other = S.bits_by_record(S.counts_exact(order=order, skip=skip, wpg=wpg))
        for g, b in other.items():
            assert np.array_equal(b, by_rec[g]), (order, skip, wpg, g)
        nomask = S.counts_exact(order=order, skip=skip, wpg=wpg, masks=False)
        assert np.array_equal(nomask["counts"], [by_rec[int(g)].sum() for g in nomask["gi"]]), (order, skip, wpg)
    for name, done in S.done_states(PATHS.index(path)).items():
        for wpg in (0, 1):
            res = S.counts_exact(done=done, wpg=wpg)
            S.check_bits(res, done)
            for j, g in enumerate(res["gi"]):
                sl = slice(ref["off"][g], ref["off"][g + 1])
                opn = done[g // S.N, ref["ty"][sl], ref["tx"][sl]] == 0
                assert np.array_equal(res["bits"][j], by_rec[int(g)] & opn), (name, wpg, j)
            nomask = S.counts_exact(done=done, wpg=wpg, masks=False)
            assert np.array_equal(nomask["counts"], res["counts"]), (name, wpg)
        if name == "one sub-pose closed":
            assert (res["counts"][res["gi"] >= S.N] == 0).all() and res["counts"].sum() > 0
    for wpg in (0, 1):
        S.counts_exact(wpg=wpg, gate=0)
        gated = S.counts_exact(wpg=wpg, gate=1)
        assert np.array_equal(gated["counts"], base["counts"])


@pytest.mark.parametrize("t_ro", [0.0, 1.0 / 30])
@pytest.mark.parametrize("exposure", [(0.0, 0.0), (-1.0 / 120, 1.0 / 120)])
@pytest.mark.parametrize("path", SWEPT_PATHS)
def test_exact_counts_swept(gs, dev, path, exposure, t_ro):
    """gs_slice_counts_exact_swept against the swept references: pixel velocities up to 300 px/s per axis"""
    S = scene_for(gs, dev, path)
    sweep = dict(t_min=exposure[0], t_max=exposure[1], t_ro=t_ro)
    base = S.counts_exact(sweep=sweep)
    kept, nstrict = S.check_bits(base, None, sweep)
    by_rec = S.bits_by_record(base)
    assert kept > 0 and nstrict > 0
    print(f"[swept {path} {exposure} {t_ro:.4f}] kept {kept} strict {nstrict} kept/strict {kept / nstrict:.4f}")
    for order, skip, wpg in (("designed", 0, 1), ("mixed", 3, 0)):
        for g, b in S.bits_by_record(S.counts_exact(order=order, skip=skip, wpg=wpg, sweep=sweep)).items():
            assert np.array_equal(b, by_rec[g]), (order, skip, wpg, g)
    done = S.done_states(7)["random half"]
    for wpg in (0, 1):
        res = S.counts_exact(done=done, wpg=wpg, sweep=sweep)
        S.check_bits(res, done, sweep)
    if exposure == (0.0, 0.0) and t_ro == 0.0:      # nothing moves: the static decisions
        for g, b in S.bits_by_record(S.counts_exact()).items():
            assert not (b & ~by_rec[g]).any()          # (the swept form only adds its slack)


# ---- emission ----------------------------------------------------------------------------------------------------------------
EMIT_PATHS = [PATHS[1], PATHS[3], PATHS[5], PATHS[6], PATHS[9], PATHS[10]]


def run_emit(S, res, counts, cum, n_out, masks, compact, wpg, invalid_key, hot=True):
    dev = S.dev
    keys = torch.full((GUARD + n_out + GUARD,), POISON32, dtype=torch.int32, device=dev)
    vals = torch.full((GUARD + n_out + GUARD,), POISON32, dtype=torch.int32, device=dev)
    th = torch.zeros(GUARD + P_SUB * S.T + GUARD, dtype=torch.uint8, device=dev)
    c_t = torch.from_numpy(counts.astype(np.int32)).to(dev)
    cum_t = torch.from_numpy(cum.astype(np.int32)).to(dev)
    pm = S._ptr
    S.check(S.L.gs_emit_open_intersects(len(counts), S.N, S.H, S.W, pm(res["slice_gi_t"]), pm(c_t), pm(cum_t), pm(S.rec_t),
                                        pm(res["done_t"]), pm(keys[GUARD:]), pm(vals[GUARD:]), invalid_key, compact, wpg,
                                        pm(res["words_t"]) if masks else None, pm(res["moff_t"]) if masks else None,
                                        pm(th[GUARD:]) if hot else None, S._stream()), "emit_open")
    k, v, h = keys.cpu().numpy(), vals.cpu().numpy(), th.cpu().numpy()
    for a in (k, v):
        assert (a[:GUARD] == POISON32).all() and (a[GUARD + n_out:] == POISON32).all(), "guard region written"
    assert not h[:GUARD].any() and not h[-GUARD:].any()
    return k[GUARD:GUARD + n_out].view(np.uint32).astype(np.int64), v[GUARD:GUARD + n_out].astype(np.int64), h[GUARD:-GUARD]


@pytest.mark.parametrize("path", EMIT_PATHS)
def test_emission_expands_the_bits_in_order(gs, dev, path):
    """gs_emit_open_intersects (masks: per-lane and wave-wide; no masks: compact and with invalid_key slots) and the
    unsliced gs_emit_intersects: keys p T + ty tiles_x + tx and values p N + g of the set bits in (y, x) order, tile_hot
    exactly on the tiles that receive a record with opacity > 0.999, guard regions around keys and vals"""
    S = scene_for(gs, dev, path)
    ref = S.ref()
    invalid = P_SUB * S.T
    done = S.done_states(3)["random half"]
    for dn in (None, done):
        for order in ("designed", "mixed"):
            res = S.counts_exact(order=order, done=dn)
            want_k, want_v, want_c = R.expand(res["bits"], res["gi"], S.rec, S.N, S.tx, S.T)
            assert np.array_equal(want_c, res["counts"])
            want_hot = R.tile_hot(want_k, want_v, S.rec, P_SUB * S.T)
            assert want_hot.any() and not want_hot.all()
            cum = np.concatenate([[0], np.cumsum(res["counts"])[:-1]])
            n_out = int(res["counts"].sum())
            for wpg in (0, 1):
                for masks in (True, False):
                    k, v, h = run_emit(S, res, res["counts"], cum, n_out, masks, 1, wpg, invalid)
                    assert np.array_equal(k, want_k) and np.array_equal(v, want_v), (order, wpg, masks)
                    assert np.array_equal(h, want_hot), (order, wpg, masks)
                # compact = 0: the open box tiles in (y, x) order, culled ones parked under invalid_key
                bc = R.box_counts(S.rec, res["gi"], S.N, dn, S.tx, S.ty)
                bk, bv = [], []
                for j, g in enumerate(res["gi"]):
                    sl = slice(ref["off"][g], ref["off"][g + 1])
                    opn = np.ones(sl.stop - sl.start, bool) if dn is None else dn[g // S.N, ref["ty"][sl], ref["tx"][sl]] == 0
                    key = (g // S.N) * S.T + ref["ty"][sl] * S.tx + ref["tx"][sl]
                    bk.append(np.where(res["bits"][j], key, invalid)[opn])
                    bv.append(np.full(int(opn.sum()), g))
                bcum = np.concatenate([[0], np.cumsum(bc)[:-1]])
                k, v, h = run_emit(S, res, bc, bcum, int(bc.sum()), False, 0, wpg, invalid)
                assert np.array_equal(k, np.concatenate(bk)) and np.array_equal(v, np.concatenate(bv)), (order, wpg)
                assert np.array_equal(h, want_hot), (order, wpg)
    # the unsliced emission takes the same decisions per tile
    sgi = S.orders["mixed"]
    area = S.area[sgi]
    cum = np.concatenate([[0], np.cumsum(area)[:-1]])
    n_out = int(area.sum())
    keys = torch.full((GUARD + n_out + GUARD,), POISON32, dtype=torch.int32, device=dev)
    vals = torch.full((GUARD + n_out + GUARD,), POISON32, dtype=torch.int32, device=dev)
    t = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    sgi_t, cum_t = t(sgi), t(cum)
    S.check(S.L.gs_emit_intersects(len(sgi), S.N, S.H, S.W, S._ptr(sgi_t), S._ptr(cum_t), S._ptr(S.rec_t), n_out,
                                   S._ptr(keys[GUARD:]), S._ptr(vals[GUARD:]), invalid, S._stream()), "emit")
    k, v = keys.cpu().numpy().view(np.uint32).astype(np.int64), vals.cpu().numpy().astype(np.int64)
    assert (k[:GUARD] == POISON32).all() and (k[-GUARD:] == POISON32).all() and (v[:GUARD] == POISON32).all() and \
        (v[-GUARD:] == POISON32).all()
    by_rec = S.bits_by_record(S.counts_exact())
    wk, wv = [], []
    for g in sgi:
        sl = slice(ref["off"][g], ref["off"][g + 1])
        wk.append(np.where(by_rec[int(g)], (g // S.N) * S.T + ref["ty"][sl] * S.tx + ref["tx"][sl], invalid))
        wv.append(np.full(sl.stop - sl.start, g))
    assert np.array_equal(k[GUARD:-GUARD], np.concatenate(wk)) and np.array_equal(v[GUARD:-GUARD], np.concatenate(wv))


# ---- gs_slice_counts, gs_tile_open_sat over tile-row widths ------------------------------------------------------------------
@pytest.mark.parametrize("tiles_x", [1, 63, 64, 65, 256])
def test_open_sat_and_box_counts(gs, dev, tiles_x):
    W, H = tiles_x * 16 - 3, 56
    n = 96
    rng = np.random.default_rng(tiles_x)
    splats = [(rng.random() * W, rng.random() * H, int(rng.choice([4, 16, 40, 200, 5000])), "plain") for _ in range(n)]
    S = Scene(gs, dev, (W, H), splats, seed=tiles_x)
    assert S.tx == tiles_x
    sgi, begin, prefix, ranks, gi = S.slice_of("mixed", 2)
    sgi_t = torch.from_numpy(sgi.astype(np.int32)).to(dev)
    for name, done in [("absent", None)] + list(S.done_states(tiles_x).items()):
        sat = None if done is None else S.open_tables(done)[1]
        cnt = torch.full((GUARD + len(gi) + GUARD,), POISON32, dtype=torch.int32, device=dev)
        sg = torch.full((GUARD + len(gi) + GUARD,), POISON32, dtype=torch.int32, device=dev)
        S.check(S.L.gs_slice_counts(len(gi), P_SUB, S.N, hp(begin), hp(prefix), S._ptr(sgi_t), S._ptr(S.rec_t), S._ptr(sat),
                                    S.H, S.W, S._ptr(sg[GUARD:]), S._ptr(cnt[GUARD:]), S._stream()), "slice_counts")
        c, s = cnt.cpu().numpy(), sg.cpu().numpy()
        assert np.array_equal(c[GUARD:-GUARD], R.box_counts(S.rec, gi, S.N, done, S.tx, S.ty)), name
        assert np.array_equal(s[GUARD:-GUARD], gi)
        for a in (c, s):
            assert (a[:GUARD] == POISON32).all() and (a[-GUARD:] == POISON32).all()
    # a gate of 0: the tables are not written
    sat = torch.full((P_SUB * (S.ty + 1) * (S.tx + 1),), POISON32, dtype=torch.int32, device=dev)
    ob = torch.full((P_SUB * S.ty * ((S.tx + 63) // 64),), POISON64, dtype=torch.int64, device=dev)
    d_t = torch.zeros(P_SUB * S.T, dtype=torch.uint8, device=dev)
    gate = torch.zeros(1, dtype=torch.int32, device=dev)
    S.check(S.L.gs_tile_open_sat(P_SUB, S.H, S.W, S._ptr(d_t), S._ptr(sat), S._ptr(ob), S._ptr(gate), S._stream()), "sat")
    assert bool((sat == POISON32).all()) and bool((ob == POISON64).all())


# ---- gs_slice_plan, gs_slice_plan_select -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K", [(1, 1), (1, 16), (256, 1), (256, 16), (3, 5)])
@pytest.mark.parametrize("start", [0, 0xFFFFFF00])
def test_slice_plan_against_the_integer_reference(gs, dev, P, K, start):
    from gsdeblur_amd import _lib
    from gsdeblur_amd.ops import _ptr, _stream
    L = _lib.load()
    N = 37
    rng = np.random.default_rng(P * 100 + K)
    counts = rng.integers(0, 40, (P, N))
    counts[P // 2] = 0                                     # a sub-pose with total 0
    if P > 2:
        counts[1] = 0
        counts[1, 5] = 3                                   # a sub-pose whose total is below base
    flat = counts.reshape(-1)
    cum = (start + np.concatenate([[0], np.cumsum(flat)[:-1]])) & R.M32
    total = (start + int(flat.sum())) & R.M32
    n_live = rng.integers(0, N + 5, P)
    t32 = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).to(dev)
    cum_t, tot_t, live_t, grand_t = t32(cum), t32([total]), t32(n_live), t32([123456789])
    for base in (8, 1, 4000):
        for live in (None, n_live):
            for form in ("plan", "select"):
                if form == "select" and (live is None or base != 8):
                    continue
                out = [torch.full((GUARD + n + GUARD,), POISON32, dtype=torch.int32, device=dev)
                       for n in (P * K, P * K, P, P + 1)]
                ptrs = [_ptr(o[GUARD:]) for o in out]
                if form == "plan":
                    _lib.check(L.gs_slice_plan(P, N, K, _ptr(cum_t), _ptr(tot_t), base, ptrs[0], ptrs[1], ptrs[2],
                                               None if live is None else _ptr(live_t), ptrs[3], _stream()), "plan")
                    want = R.slice_plan(P, N, K, cum, total, base, live)
                else:
                    _lib.check(L.gs_slice_plan_select(P, N, K, _ptr(cum_t), _ptr(tot_t), ptrs[0], ptrs[1], ptrs[2],
                                                      _ptr(live_t), ptrs[3], _ptr(grand_t), _stream()), "plan_select")
                    want = R.slice_plan(P, N, K, cum, total, 1 << 40, live, grand=123456789)
                    assert (want[0].reshape(P, K) == np.minimum(n_live, N)[:, None]).all()   # every boundary behind them
                for o, w, name in zip(out, want, ("bounds", "rels", "seg_totals", "tail")):
                    h = o.cpu().numpy()
                    assert np.array_equal(h[GUARD:-GUARD].view(np.uint32).astype(np.int64), w), (name, base, form)
                    assert (h[:GUARD] == POISON32).all() and (h[-GUARD:] == POISON32).all(), name


# ---- gs_exclusive_scan_segments_u32, gs_gather_counts, gs_make_depth_keys64 -----------------------------------------------
@pytest.mark.parametrize("seg_len", [1, 255, 256, 257, 2047, 2048, 2049, 5 * 256 + 1])
def test_segmented_scan_gather_and_depth_keys(gs, dev, seg_len):
    from gsdeblur_amd import _lib
    from gsdeblur_amd.ops import _ptr, _stream
    L = _lib.load()
    segs = 9
    n = segs * seg_len
    rng = np.random.default_rng(seg_len)
    x = rng.integers(0, 2 ** 31, n).astype(np.int64)             # sums wrap modulo 2^32
    cnt = rng.integers(0, seg_len + 1, segs)
    cnt[0], cnt[3], cnt[-1] = seg_len, 0, seg_len                # a full, an empty and a full last segment
    t32 = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).to(dev)
    ws_b = L.gs_scan_workspace_bytes(n)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    out = torch.full((GUARD + n + GUARD,), POISON32, dtype=torch.int32, device=dev)
    tot = torch.full((3,), POISON32, dtype=torch.int32, device=dev)
    cnt_t, x_t = t32(cnt), t32(x)
    _lib.check(L.gs_exclusive_scan_segments_u32(n, seg_len, _ptr(cnt_t), _ptr(x_t), _ptr(out[GUARD:]), _ptr(tot[1:]),
                                                _ptr(ws), ws_b, _stream()), "segmented scan")
    want, defined, total = R.segmented_exclusive_scan(x, seg_len, cnt)
    h = out.cpu().numpy()
    got = h[GUARD:-GUARD].view(np.uint32).astype(np.int64)
    assert np.array_equal(got[defined], want[defined])
    assert (h[:GUARD] == POISON32).all() and (h[-GUARD:] == POISON32).all()
    th = tot.cpu().numpy().view(np.uint32)
    assert int(th[1]) == total and th[0] == POISON32 and th[2] == POISON32
    # gather_counts and depth_keys64 over the same n
    sgi = rng.permutation(n)
    nt = rng.integers(0, 5000, n)
    o32 = torch.full((GUARD + n + GUARD,), POISON32, dtype=torch.int32, device=dev)
    sgi_t, nt_t = t32(sgi), t32(nt)
    _lib.check(L.gs_gather_counts(n, _ptr(sgi_t), _ptr(nt_t), _ptr(o32[GUARD:]), _stream()), "gather")
    h = o32.cpu().numpy()
    assert np.array_equal(h[GUARD:-GUARD].view(np.uint32).astype(np.int64), R.gather_counts(sgi, nt))
    assert (h[:GUARD] == POISON32).all() and (h[-GUARD:] == POISON32).all()
    o64 = torch.full((GUARD + n + GUARD,), POISON64, dtype=torch.int64, device=dev)
    N = max(seg_len // 2, 1)
    _lib.check(L.gs_make_depth_keys64(n, N, _ptr(x_t), _ptr(o64[GUARD:]), _stream()), "keys64")
    h = o64.cpu().numpy().view(np.uint64)
    assert np.array_equal(h[GUARD:-GUARD], R.depth_keys64(x, N))
    assert (h[:GUARD] == POISON64).all() and (h[-GUARD:] == POISON64).all()


# ---- gs_reduce_grad_tuples -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mult", [1, 3])
@pytest.mark.parametrize("form", ["thread per Gaussian (n_isect <= 32 n_slice)", "wave per Gaussian (n_isect > 32 n_slice)"])
def test_reduce_grad_tuples_against_a_float64_sum(gs, dev, form, mult):
    """synthetic tuples and flags: counts 0, 1, 15, 16, 17, 63, 64, 65 and a few thousand; unflagged tuples are ignored;
    flags == 2 divides slot 5 by -opacity; `touched` exactly where something was written; other rows keep their NaN; two
    runs bit-identical.  Tolerance (derived): a float32 sum of n terms in any fixed order differs from the exact sum by at
    most n 2^-24 sum|x|; the flags == 2 slot adds the reciprocal (1 ulp) and one product: 2^-22 |result|."""
    from gsdeblur_amd import _lib
    from gsdeblur_amd.ops import _ptr, _stream
    L = _lib.load()
    rng = np.random.default_rng(len(form) + mult)
    counts = [0, 1, 15, 16, 17, 63, 64, 65, 3000, 0, 2100, 5]
    if form.startswith("thread"):
        counts += list(rng.integers(0, 3, 400))
    counts = np.array(counts, np.int64)
    rng.shuffle(counts)
    ns, rows = len(counts), 2 * len(counts) + 7
    n_isect = int(counts.sum())
    assert (n_isect > 32 * ns) == form.startswith("wave")
    cum = np.concatenate([[0], np.cumsum(counts)[:-1]])
    slice_gi = rng.permutation(rows)[:ns]
    tuples = (rng.standard_normal((n_isect * mult, 12)) * np.exp(rng.standard_normal((n_isect * mult, 1)) * 3)).astype(np.float32)
    flags = (rng.random(n_isect * mult) < 0.7).astype(np.uint8)
    raw_g = rng.random(ns) < 0.5                                  # Gaussians whose flagged tuples carry the value 2
    owner = np.repeat(np.arange(ns), counts * mult)
    flags[(flags == 1) & raw_g[owner]] = 2
    one = int(np.nonzero(counts == 1)[0][0])
    flags[cum[one] * mult:(cum[one] + 1) * mult] = 0              # a Gaussian with tuples, none flagged: nothing written
    rec = np.zeros((rows, 16), np.float32)
    rec[:, 5] = rng.uniform(0.05, 1.0, rows)
    want = np.full((rows, 12), np.nan)
    tol = np.zeros((rows, 12))
    wrote = np.zeros(rows, np.uint8)
    for j in range(ns):
        sl = slice(int(cum[j]) * mult, int(cum[j] + counts[j]) * mult)
        f = flags[sl] != 0
        if not f.any():
            continue
        x = tuples[sl][f].astype(np.float64)
        g = slice_gi[j]
        want[g, :11], want[g, 11] = x[:, :11].sum(0), 0.0
        tol[g, :11] = len(x) * 2.0 ** -24 * np.abs(x[:, :11]).sum(0)
        if (flags[sl] == 2).any():
            op = float(rec[g, 5])
            want[g, 5], tol[g, 5] = -want[g, 5] / op, tol[g, 5] / op
            tol[g, 5] += 2.0 ** -22 * abs(want[g, 5])
        wrote[g] = 1
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
    gi_t, c_t, cum_t, tup_t, fl_t, rec_t = (t(slice_gi, np.int32), t(counts, np.int32), t(cum, np.int32), t(tuples, np.float32),
                                            t(flags, np.uint8), t(rec, np.float32))
    runs = []
    for _ in range(2):
        v = torch.full((GUARD + rows * 12 + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        touched = torch.zeros(GUARD + rows + GUARD, dtype=torch.uint8, device=dev)
        _lib.check(L.gs_reduce_grad_tuples(ns, _ptr(gi_t), _ptr(c_t), _ptr(cum_t), _ptr(tup_t), _ptr(fl_t), _ptr(v[GUARD:]),
                                           _ptr(touched[GUARD:]), n_isect, _ptr(rec_t), mult, _stream()), "reduce")
        vh, th = v.cpu().numpy(), touched.cpu().numpy()
        assert np.isnan(vh[:GUARD]).all() and np.isnan(vh[-GUARD:]).all() and not th[:GUARD].any() and not th[-GUARD:].any()
        assert np.array_equal(th[GUARD:-GUARD], wrote)
        got = vh[GUARD:-GUARD].reshape(rows, 12).astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))       # rows of other Gaussians keep their NaN
        ok = ~np.isnan(want)
        excess = np.abs(got[ok] - want[ok]) - tol[ok]
        assert (excess <= 0).all(), float(excess.max())
        runs.append(vh.view(np.uint32).copy())
    assert np.array_equal(runs[0], runs[1])


# ---- one render: the bits against the compositor ---------------------------------------------------------------------------
def _g1_cut():
    geom = (256, 64)
    sp = [(60.0, 30.0, 24), (120.0, 20.0, 48), (200.0, 40.0, 56), (30.0, 50.0, 32), (128.0, 32.0, 120), (90.0, 10.0, 64)]
    return geom, wave(geom, sp)


@pytest.mark.parametrize("which", ["G3", "256 x 64 cut of the G1 classes"])
def test_culled_lists_render_the_same_image(gs, dev, which):
    """gs_rasterize_fwd over the full box lists and over the lists culled by the exact count's bits: image and out_T are
    bit-identical (a culled pair has alpha < 1/255 at every pixel of its tile, so the compositor skips it anyway)"""
    from gsdeblur_amd import ops
    geom, splats = (G3, spec_for("partial tiles both ways")[1]) if which == "G3" else _g1_cut()
    S = Scene(gs, dev, geom, splats, seed=77)
    res = S.counts_exact()
    assert sum(int(b.sum()) for b in res["bits"]) < int(S.area[res["gi"]].sum())          # something is culled
    outs = []
    for bits in ([np.ones(int(S.area[g]), bool) for g in res["gi"]], res["bits"]):
        keys, vals, _ = R.expand(bits, res["gi"], S.rec, S.N, S.tx, S.T)
        order = np.argsort(keys, kind="stable")                        # per tile, depth (emission) order kept
        ids = torch.zeros(len(keys) + ops.IDS_PAD, dtype=torch.int32, device=dev)
        ids[:len(keys)] = torch.from_numpy(vals[order].astype(np.int32)).to(dev)
        t_ids = np.arange(P_SUB * S.T)
        bins = np.stack([np.searchsorted(keys[order], t_ids, "left"), np.searchsorted(keys[order], t_ids, "right")], 1)
        bins_t = torch.from_numpy(bins.astype(np.int32)).to(dev)
        bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
        edges = ops._band_edges(S.H, 1, dev)
        img = torch.full((P_SUB, S.H, S.W, 3), -1.0, device=dev)
        out_T = torch.full((P_SUB, S.H, S.W), -1.0, device=dev)
        fidx = torch.zeros(P_SUB, S.H, S.W, dtype=torch.int32, device=dev)
        S.check(S.L.gs_rasterize_fwd(S._ptr(S.rec_t), S._ptr(ids), S._ptr(bins_t), S._ptr(edges), S._ptr(bg), P_SUB, 1, S.H,
                                     S.W, S._ptr(img), S._ptr(out_T), S._ptr(fidx), P_SUB * S.N, 0, S._stream()), "fwd")
        outs.append((img.cpu().numpy().view(np.uint32), out_T.cpu().numpy().view(np.uint32)))
    assert float(outs[0][1].view(np.float32).min()) < 0.9                                  # the splats were blended
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
