"""The exact tile cull's ellipse test on the CPU: csrc/tilecull_math.h compiled with g++ (tests/host_math/tilecull_host.cpp)
against the float64 definitions of tests/slicefront_reference.py over a seeded fuzz of 10^5 ellipses, static and swept,
and the reference's own integer restatements on hand-checked cases.

Two caps, both zero: (a) no strict pair (a pixel centre of the tile inside the image with alpha >= 1/255) is culled;
(b) no kept pair of a well-conditioned conic (det >= 1e-3 a c) lies outside loose_hit (twice the documented slack).
A cull that never culls fails (b); a cull that drops a corner tile fails (a)."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import slicefront_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "tilecull_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libtilecull_host.so"
CSRC = ROOT / "3dgs-deblur_amd" / "csrc"
HDRS = [CSRC / "tilecull_math.h", CSRC / "gs_math.h"]

W, H = 2048, 200                       # 128 x 13 tiles, the last tile row 8 pixels high
N_ELLIPSES = 100_000
SWEEP = dict(t_min=-1.0 / 120, t_max=1.0 / 120, t_ro=1.0 / 30)


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def load_host():
    if not LIB.exists() or LIB.stat().st_mtime < max(f.stat().st_mtime for f in [SRC, *HDRS]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{CSRC}", str(SRC),
                               "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.tc_hits.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                            ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.tc_derived.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_bits(lib, rec, Wi, Hi, sweep=None, by_row=0):
    """the header's decision for every pair of R.box_pairs(rec), in that order"""
    rec = np.ascontiguousarray(rec, np.float32)
    off = np.ascontiguousarray(R.box_pairs(rec)[0], np.int64)
    out = np.full(int(off[-1]) + 1, 7, np.uint8)
    pv = None if sweep is None else np.ascontiguousarray(sweep["pix_vel"], np.float32)
    rc = lib.tc_hits(len(rec), P(rec), Wi, Hi, 0 if sweep is None else 1, None if pv is None else P(pv),
                     0.0 if sweep is None else sweep["t_min"], 0.0 if sweep is None else sweep["t_max"],
                     0.0 if sweep is None else sweep["t_ro"], by_row, P(off), P(out))
    assert rc == 0 and out[-1] == 7
    return out[:-1].astype(bool)


@pytest.fixture(scope="module")
def th():
    return load_host()


def fuzz_records(n, seed, sweep_pad=0.0):
    """major axis 0.3 .. 6000 px (log-uniform), anisotropy up to 2e4 (log-uniform) with the minor axis floored at 0.3 px,
    any angle; centres on screen / up to 40 px off screen / 2e4 px away; opacity (1/255) [1, 1.05] / [0.999, 1] / uniform"""
    rng = np.random.default_rng(seed)
    s1 = 0.3 * np.exp(rng.random(n) * np.log(6000 / 0.3))
    s2 = np.maximum(s1 / np.exp(rng.random(n) * np.log(2e4)), 0.3)
    th_ = rng.random(n) * 2 * np.pi
    cs, sn, l1, l2 = np.cos(th_), np.sin(th_), s1 * s1, s2 * s2
    cxx, cxy, cyy = cs * cs * l1 + sn * sn * l2, cs * sn * (l1 - l2), sn * sn * l1 + cs * cs * l2
    det = l1 * l2
    conic = np.stack([cyy / det, -cxy / det, cxx / det], 1).astype(np.float32)
    where = rng.integers(0, 3, n)
    xy = np.stack([rng.random(n) * W, rng.random(n) * H], 1)
    off = where == 1
    xy[off, 0] = np.where(rng.random(off.sum()) < 0.5, -rng.random(off.sum()) * 40, W + rng.random(off.sum()) * 40)
    xy[off, 1] = np.where(rng.random(off.sum()) < 0.5, -rng.random(off.sum()) * 40, H + rng.random(off.sum()) * 40)
    far = where == 2
    xy[far, 0] += np.where(rng.random(far.sum()) < 0.5, -2e4, 2e4)
    xy[far, 1] += np.where(rng.random(far.sum()) < 0.5, -2e4, 2e4) * (rng.random(far.sum()) < 0.5)
    band = rng.integers(0, 3, n)
    op = np.where(band == 0, (1 / 255) * (1 + 0.05 * rng.random(n)), np.where(band == 1, 0.999 + 0.001 * rng.random(n),
                                                                               rng.random(n)))
    op = np.minimum(op.astype(np.float32), np.float32(1.0))
    xy = xy.astype(np.float32)
    rec = R.make_records(xy, conic, op, R.circle_box(xy, np.ceil(3 * s1), W, H, pad=sweep_pad))
    pv = ((rng.random((n, 2)) - 0.5) * 800).astype(np.float32)
    return rec, pv


def run_fuzz(lib, sweep, chunk=4000, stats_every=1):
    """-> dict(pairs, strict, kept, kept_of_checked, culled_strict, kept_not_loose, forms_differ).  (a) is evaluated on EVERY
    culled pair; the strict count (for the ratio kept / strict) on every stats_every-th record."""
    pad = 0.0
    if sweep is not None:
        pad = 400 * np.sqrt(2) * (max(abs(sweep["t_min"]), abs(sweep["t_max"])) + 0.5 * abs(sweep["t_ro"])) + 1
    rec_all, pv_all = fuzz_records(N_ELLIPSES, 20250 + (sweep is not None), pad)
    tot = dict(pairs=0, strict=0, kept=0, kept_of_checked=0, culled_strict=0, kept_not_loose=0, forms_differ=0,
               well_conditioned_kept=0)
    for s0 in range(0, N_ELLIPSES, chunk):
        rec = rec_all[s0:s0 + chunk]
        sw = None if sweep is None else dict(sweep, pix_vel=pv_all[s0:s0 + chunk])
        _, ri, tx, ty = R.box_pairs(rec)
        kept = host_bits(lib, rec, W, H, sw, 0)
        tot["forms_differ"] += int((kept != host_bits(lib, rec, W, H, sw, 1)).sum())
        checked = (ri + s0) % stats_every == 0
        strict = R.strict_hits(rec, ri, tx, ty, W, H, sw, only=(~kept) | checked)
        tot["culled_strict"] += int((strict & ~kept).sum())
        tot["strict"] += int((strict & checked).sum())
        tot["kept_of_checked"] += int((kept & checked).sum())
        wc = R.well_conditioned(rec)[ri] & kept
        idx = np.nonzero(wc)[0]
        loose = R.loose_hits(rec, ri[idx], tx[idx], ty[idx], W, H, sw)
        tot["kept_not_loose"] += int((~loose).sum())
        tot["well_conditioned_kept"] += int(idx.size)
        tot["pairs"] += len(ri)
        tot["kept"] += int(kept.sum())
    return tot


def test_static_fuzz_keeps_every_strict_pair_and_nothing_beyond_the_loose_set(th):
    t = run_fuzz(th, None)
    print("static fuzz:", t, "kept/strict = %.4f" % (t["kept_of_checked"] / max(t["strict"], 1)))
    assert t["pairs"] > 10 ** 7 and t["strict"] > 10 ** 6
    assert t["forms_differ"] == 0                 # tile_hit per tile == row_span + span_tiles over the box row
    assert t["culled_strict"] == 0                # (a)
    assert t["kept_not_loose"] == 0               # (b)
    assert t["kept"] < 0.5 * t["pairs"]           # the cull culls


def test_swept_fuzz_keeps_every_strict_pair_and_nothing_beyond_the_loose_set(th):
    """pixel velocities up to 400 px/s per axis, exposure [-1/120, 1/120], readout 1/30.  (a) over every culled pair; the
    strict count behind the printed ratio over every 16th record (256 pixels x a time interval per pair)."""
    t = run_fuzz(th, SWEEP, stats_every=16)
    print("swept fuzz:", t, "kept/strict (every 16th record) = %.4f" % (t["kept_of_checked"] / max(t["strict"], 1)))
    assert t["pairs"] > 10 ** 7 and t["strict"] > 5 * 10 ** 4
    assert t["forms_differ"] == 0
    assert t["culled_strict"] == 0
    assert t["kept_not_loose"] == 0
    assert t["kept"] < 0.5 * t["pairs"]


def test_row_form_of_strict_equals_the_pixel_definition(th):
    """the reference against itself: the closed-form row minimiser and the candidate pre-filter give the brute-force
    answer (all 256 pixels), on pairs near the ellipse edge where they could differ; partial tiles both ways"""
    for (Wi, Hi, n, seed) in ((W, H, 300, 1), (40, 24, 300, 2)):
        rec, pv = fuzz_records(n, seed)
        if Wi != W:
            rec[:, 0] *= Wi / W
            rec[:, 1] *= Hi / H
            rec = R.make_records(rec[:, 0:2], rec[:, 2:5], rec[:, 5], R.circle_box(rec[:, 0:2], np.full(n, 40.0), Wi, Hi))
        _, ri, tx, ty = R.box_pairs(rec)
        near = R.strict_candidates(rec, ri, tx, ty, Wi, Hi)
        pick = np.nonzero(near)[0][:6000]
        far = np.nonzero(~near)[0][:2000]
        brute = R._strict_pixels(rec, ri[pick], tx[pick], ty[pick], Wi, Hi)
        fast = R.strict_hits(rec, ri, tx, ty, Wi, Hi)
        assert np.array_equal(fast[pick], brute) and brute.any() and not brute.all()
        assert not R._strict_pixels(rec, ri[far], tx[far], ty[far], Wi, Hi).any()
        sw = dict(SWEEP, pix_vel=pv)
        near = R.strict_candidates(rec, ri, tx, ty, Wi, Hi, sw)
        far = np.nonzero(~near)[0][:1500]
        assert not R._strict_pixels(rec, ri[far], tx[far], ty[far], Wi, Hi, sw).any()


def test_single_pair_forms_and_hand_cases(th):
    # a round splat of sigma 4 px at the centre of tile (2, 1), opacity 0.5: ln(127.5) = 4.848 -> reach 4 sqrt(2 * 4.848) =
    # 12.46 px: from (40, 24) it reaches pixel centre 31.5 (tile 1: 8.5 px away) but not tile 0 (24.5 px), nor row 3
    rec = R.make_records(np.array([[40.0, 24.0]]), np.array([[1 / 16, 0.0, 1 / 16]]), np.array([0.5]),
                         (np.array([0]), np.array([0]), np.array([5]), np.array([4])))
    got = host_bits(th, rec, 80, 64).reshape(4, 5)
    want = np.zeros((4, 5), bool)
    want[0:3, 1:4] = True
    assert np.array_equal(got, want)
    for ty in range(4):
        for tx in range(5):
            assert R.strict_hit(rec[0], tx, ty, 80, 64) == want[ty, tx]
            assert R.loose_hit(rec[0], tx, ty, 80, 64) == want[ty, tx]
    # moving at 900 px/s in x for 1/60 s either way (15 px): tiles 0 and 4 of the middle rows come into reach (9.5 px)
    sw = dict(pix_vel=np.array([[900.0, 0.0]], np.float32), t_min=-1 / 60, t_max=1 / 60, t_ro=0.0)
    got = host_bits(th, rec, 80, 64, sw).reshape(4, 5)
    assert got[1, 0] and got[1, 4] and not got[3].any()
    assert R.strict_hit(rec[0], 0, 1, 80, 64, sw) and not R.strict_hit(rec[0], 0, 3, 80, 64, sw)
    # opacity at and below 1/255, a degenerate conic
    rec2 = np.repeat(rec, 3, 0)
    rec2[0, 5], rec2[1, 5] = np.float32(1 / 255) * np.float32(0.99), 0.0
    rec2[2, 2:5] = (1.0, 1.0, 1.0)                     # det = 0: never culled
    got = host_bits(th, rec2, 80, 64).reshape(3, 20)
    assert not got[0].any() and not got[1].any() and got[2].all()
    d = np.zeros(12, np.float32)
    assert th.tc_derived(3, P(np.ascontiguousarray(rec2)), P(d)) == 0
    assert d[0] == -1 and d[4] == -1 and d[9] > 1e37


# Needles the static fuzz found (2048 x 200, full-screen boxes): det / (a c) between 1e-7 and 7e-7, inside the rounding error
# of the float32 determinant.  With the plain float32 a c - b b each of them lost one to three tiles that hold a pixel with
# alpha >= 1/255.  (x, y, conic a, b, c, opacity), float32 values
NEEDLES = [(-4.4871583, 232.17252, 1.327560305595398, 3.603921890258789, 9.783551216125488, 0.004055326),
           (2051.6611, 224.98425, 1.237034797668457, -3.4949355125427246, 9.874076843261719, 0.0040615117),
           (-39.195515, 204.34195, 1.333858847618103, 3.179032564163208, 7.576701641082764, 0.004083189),
           (1003.9277, 192.6448, 1.1115189790725708, 2.7974283695220947, 7.040461540222168, 0.0039763656),
           (1312.296, 126.09779, 1.816888451576233, 4.109325408935547, 9.29422378540039, 0.00410558),
           (-10.243413, -9.645885, 0.14811745285987854, -1.055833339691162, 7.52635383605957, 0.00409739),
           (1137.9934, 16.156992, 1.9827345609664917, 4.185582637786865, 8.835829734802246, 0.0039774645)]


def test_needles_whose_determinant_is_rounding_noise_lose_no_strict_tile(th):
    v = np.array(NEEDLES, np.float32)
    n = len(v)
    full = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, 128), np.full(n, 13))
    rec = R.make_records(v[:, 0:2], v[:, 2:5], v[:, 5], full)
    _, ri, tx, ty = R.box_pairs(rec)
    kept = host_bits(th, rec, W, H)
    strict = R.strict_hits(rec, ri, tx, ty, W, H)
    assert np.array_equal(strict, R._strict_pixels(rec, ri, tx, ty, W, H))
    assert strict.sum() > 100 and not (strict & ~kept).any()
    assert not R.well_conditioned(rec).any()


def test_integer_restatements_on_hand_cases():
    # slice plan: P = 2, N = 4, counts (3, 0, 5, 2 | 1, 1, 0, 7), prefix wrapping past 2^32
    counts = np.array([3, 0, 5, 2, 1, 1, 0, 7])
    start = 0xFFFFFFFA
    cum = (start + np.concatenate([[0], np.cumsum(counts)[:-1]])) & R.M32
    total = (start + counts.sum()) & R.M32
    b, r, s, t = R.slice_plan(2, 4, 2, cum, total, 4)
    assert b.tolist() == [3, 3, 4, 4] and r.tolist() == [8, 8, 9, 9] and s.tolist() == [10, 9] and t.tolist() == [4, 4, total]
    b, r, s, t = R.slice_plan(2, 4, 1, cum, total, 1, n_live=[2, 9], grand=77)
    assert b.tolist() == [1, 1] and r.tolist() == [3, 1] and t.tolist() == [2, 4, 77]
    # summed-area table and open bits: 3 x 2 tiles, tile (1, 0) closed
    done = np.zeros((1, 2, 3), np.uint8)
    done[0, 0, 1] = 1
    sat, bits = R.open_sat(done, 1, 3, 2)
    assert sat[0].tolist() == [[0, 0, 0, 0], [0, 1, 1, 2], [0, 2, 3, 5]] and bits[0, :, 0].tolist() == [0b101, 0b111]
    rec = R.make_records(np.zeros((2, 2)), np.ones((2, 3)), np.ones(2), (np.array([0, 1]), np.array([0, 0]),
                                                                          np.array([3, 3]), np.array([2, 1])))
    assert R.box_counts(rec, np.array([0, 1]), 2, done, 3, 2).tolist() == [5, 1]
    assert R.box_counts(rec, np.array([1, 0]), 2, None, 3, 2).tolist() == [2, 6]
    # mask words: areas (6, 2) in rank order; slice = ranks (1, 0)
    cum_rank, moff, nw = R.mask_layout(rec, np.array([0, 1]), np.array([1, 0]))
    assert cum_rank.tolist() == [0, 6] and moff.tolist() == [0, 1] and nw.tolist() == [1, 1]
    bits_of = [np.array([True, False]), np.array([True, False, False, False, True, True])]
    k, v, c = R.expand(bits_of, np.array([1, 0]), rec, 2, 3, 6)
    assert k.tolist() == [1, 0, 4, 5] and v.tolist() == [1, 0, 0, 0] and c.tolist() == [1, 3]
    rec[0, 5], rec[1, 5] = 0.9995, 0.999
    assert R.tile_hot(k, v, rec, 6).tolist() == [1, 0, 0, 0, 1, 1]
    out, defined, total = R.segmented_exclusive_scan([5, 6, 7, 8, 9, 10], 3, [2, 0])
    assert out[defined].tolist() == [0, 5, 11] and total == 11
    assert R.gather_counts([2, 0], [4, 5, 6]).tolist() == [6, 4]
    assert R.depth_keys64([9, 8, 7], 2).tolist() == [9, 8, (1 << 32) | 7]
    word = np.array([0b1011, 0], np.uint64)
    inside, beyond = R.unpack_mask(word, 0, 3)
    assert inside.tolist() == [True, True, False] and beyond[0] and not beyond[1:].any()
