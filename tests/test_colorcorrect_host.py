"""Colour-corrected metrics on the CPU: csrc/colorcorrect_math.h compiled with g++ against the float64 reference
(tests/colorcorrect_reference.py), color_correct_torch against the same reference at the GPU test's sizes, answers known
without the reference, evaluate() on a stand-in render, and the C-ABI entries.

Tolerance of the comparisons with the reference (colorcorrect_reference.check_case, the rule of
tests/test_gpu_colorcorrect.py): 4 x the largest difference between reference(store=float32) and reference(store=None) on
the same inputs, plus 1e-6; cases up to 64 x 48 have no pixel within 1e-6 of a mask threshold (asserted)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import colorcorrect_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "colorcorrect_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libcolorcorrect_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "colorcorrect_math.h"
HIP = ROOT / "3dgs-deblur_amd" / "csrc" / "colorcorrect.hip"
NEW_EXPORTS = {"gs_color_correct_workspace_bytes": 3, "gs_color_correct": 12}
TILE = int(re.search(r"constexpr int kTile = (\d+);", HIP.read_text()).group(1))     # the moments kernel's pixel tile
ROWS = [(TILE - 1, 1), (TILE, 1), (TILE + 1, 1)]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def ch():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", f"-I{HDR.parent}",
                               str(SRC), "-o", str(LIB)])
    lib = ctypes.CDLL(str(LIB))
    lib.ch_row_masks.restype = ctypes.c_uint
    lib.ch_row_masks.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_double]
    lib.ch_moments.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 3 + [ctypes.c_double, ctypes.c_void_p]
    lib.ch_color_correct.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                     ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _host_fit(ch, img, ref, num_iters=5, eps=R.EPS):
    B, H, W, _ = img.shape
    out = np.zeros((B, H, W, 3), np.float32)
    warps = np.zeros((B, num_iters, 3, 10), np.float64)
    for b in range(B):
        i, r = (np.ascontiguousarray(t[b].numpy()) for t in (img, ref))
        o, w = np.zeros_like(i), np.zeros((num_iters, 3, 10))
        ch.ch_color_correct(H * W, P(i), P(r), num_iters, eps, P(o), P(w))
        out[b], warps[b] = o, w
    return torch.from_numpy(out), torch.from_numpy(warps)


# ---- host-compiled math ---------------------------------------------------------------------------------------------
def test_header_feature_order_and_gram_index(ch):
    x = np.array([0.25, 0.5, 0.75], np.float32)
    a = np.zeros(10)
    ch.ch_features(P(x), P(a))
    assert a.tolist() == [0.0625, 0.125, 0.1875, 0.25, 0.375, 0.5625, 0.25, 0.5, 0.75, 1.0]
    assert a.tolist() == R.features(x).tolist()
    k = 0
    for i in range(10):
        for j in range(i, 10):
            assert ch.ch_gram_index(i, j) == k
            k += 1
    assert k == 55


def test_header_masks_are_float32_compares_against_the_rounded_thresholds(ch):
    lo, hi = R.thresholds()
    mid = np.float32(0.5)
    below, above = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))
    assert float(lo) != R.EPS and float(hi) != 1.0 - R.EPS              # the thresholds ARE rounded

    def m(img, x, ref):
        return ch.ch_row_masks(*(P(np.array(v, np.float32)) for v in (img, x, ref)), R.EPS)
    assert m([mid] * 3, [mid] * 3, [mid] * 3) == 7
    assert m([lo, hi, mid], [hi, lo, lo], [mid, mid, hi]) == 7          # both ends are inside
    assert m([below, mid, mid], [mid, mid, mid], [mid, mid, mid]) == 6  # channel 0 out by the original image
    assert m([mid, mid, mid], [mid, above, mid], [mid, mid, mid]) == 5  # channel 1 out by the current image
    assert m([mid, mid, mid], [mid, mid, mid], [mid, mid, 0.0]) == 3    # channel 2 out by the reference
    assert m([mid] * 3, [mid, np.nan, mid], [mid] * 3) == 5


def test_header_moments_and_solve_against_the_reference_and_lstsq(ch):
    img, ref = R.random_case(1, 12, 16, 11)
    i, r = (np.ascontiguousarray(t[0].numpy()).reshape(-1, 3) for t in (img, ref))
    sums = np.zeros((3, 65))
    ch.ch_moments(len(i), P(i), P(i), P(r), R.EPS, P(sums))
    lo, hi = R.thresholds()
    mask = (i >= lo) & (i <= hi) & (r >= lo) & (r <= hi)
    assert 0 < mask.sum() < mask.size                                    # some pixels are saturated
    for c in range(3):
        G, h = R.moments(i, mask[:, c], r[:, c])
        assert sums[c, 54] == mask[:, c].sum()                           # the count is G[9][9]
        assert np.allclose(sums[c, :55], G[np.triu_indices(10)], rtol=1e-13, atol=0)
        assert np.allclose(sums[c, 55:], h, rtol=1e-13, atol=0)
        w = np.zeros(10)
        assert ch.ch_solve(P(np.ascontiguousarray(sums[c])), c, P(w)) == 1
        w_ref, fitted = R.solve_channel(G, h, c)
        assert fitted and np.allclose(w, w_ref, rtol=0, atol=1e-11)
        a = R.features(i)[mask[:, c]]
        w_lstsq = np.linalg.lstsq(a, r[mask[:, c], c].astype(np.float64), rcond=None)[0]
        print(f"channel {c}: |w - lstsq| {np.abs(w - w_lstsq).max():.2e}, cond(a) {np.linalg.cond(a):.0f}")
        assert np.allclose(w, w_lstsq, rtol=0, atol=1e-9)


def test_header_degenerate_rule(ch):
    w = np.zeros(10)
    a = R.features(np.random.default_rng(0).uniform(0.1, 0.9, (9, 3)))
    sums = np.concatenate([(a.T @ a)[np.triu_indices(10)], a.T @ np.full(9, 0.5)])
    assert ch.ch_solve(P(sums), 1, P(w)) == 0 and w.tolist() == R.identity_warp(1).tolist()       # nine rows
    a = R.features(np.full((50, 3), 0.5))
    sums = np.concatenate([(a.T @ a)[np.triu_indices(10)], a.T @ np.full(50, 0.25)])
    assert ch.ch_solve(P(sums), 2, P(w)) == 0 and w.tolist() == R.identity_warp(2).tolist()       # rank one
    assert R.solve_channel(a.T @ a, a.T @ np.full(50, 0.25), 2)[1] is False
    x = np.random.default_rng(1).uniform(0.1, 0.9, (50, 1)).repeat(3, 1)                          # grey: rank three
    a = R.features(x)
    sums = np.concatenate([(a.T @ a)[np.triu_indices(10)], a.T @ x[:, 0]])
    assert ch.ch_solve(P(sums), 0, P(w)) == 0 and w.tolist() == R.identity_warp(0).tolist()
    sums[:] = np.nan
    assert ch.ch_solve(P(sums), 0, P(w)) == 0 and w.tolist() == R.identity_warp(0).tolist()


@pytest.mark.parametrize("size", R.SIZES[:4] + ROWS)
def test_header_fit_against_the_reference(ch, size):
    W, H = size
    for B in (1, 3):
        k = R.case(B, H, W)
        out, warps = _host_fit(ch, k["img"], k["ref"])
        R.check_case(k, out, warps, f"host {W}x{H} B={B}")


# ---- the torch restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.SIZES + ROWS)
def test_torch_restatement_against_the_reference(gs, size):
    W, H = size
    for B in (1, 3):
        k = R.case(B, H, W)
        out, warps = gs.colorcorrect.color_correct_torch(k["img"], k["ref"], return_warps=True)
        assert out.dtype == torch.float32 and out.shape == k["img"].shape and warps.shape == (B, 5, 3, 10)
        R.check_case(k, out, warps, f"torch {W}x{H} B={B}")
    one = gs.color_correct(k["img"][1], k["ref"][1])                      # CPU tensors take the restatement
    assert one.shape == (H, W, 3) and float((one - out[1]).abs().max()) <= 1e-6   # torch's batched matmul sums differently


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_an_image_fitted_to_itself_comes_back(gs):
    img = R.random_case(1, 12, 16, 3)[0][0]
    out, warps = gs.color_correct(img, img.clone(), return_warps=True)
    assert float((out - img).abs().max()) <= 1e-6
    assert float((warps - gs.colorcorrect.identity_warps(1, 5)[0]).abs().max()) <= 1e-6


def test_an_exact_unclipped_quadratic_warp_is_recovered(gs):
    g = torch.Generator().manual_seed(9)
    img = (0.3 + 0.4 * torch.rand(12, 16, 3, generator=g, dtype=torch.float64)).float()
    a = torch.from_numpy(R.features(img.numpy()))
    Wt = torch.tensor([[0.2, 0, 0, 0, 0, 0, 0.8, 0.1, 0, 0.01],                # rr, r, g, 1
                       [0, 0, 0, 0, -0.15, 0, 0, 1.05, 0, 0.02],               # gb, g, 1
                       [0, 0, 0, 0, 0, 0.1, 0.05, 0, 0.85, -0.01]], dtype=torch.float64)   # bb, r, b, 1
    ref = (a @ Wt.T).float()
    assert 0.2 <= float(ref.min()) and float(ref.max()) <= 0.8 and 0.2 <= float(img.min()) and float(img.max()) <= 0.8
    out, warps = gs.color_correct(img, ref, return_warps=True)
    err = float((out - ref).abs().max())
    print(f"exact quadratic warp: max |out - ref| = {err:.2e}")
    assert err <= 2.0 ** -23                          # float32 rounding of values below 1, twice (ref's and out's)
    assert float((warps[0] - Wt).abs().max()) <= 1e-5  # ref was rounded to float32: the first fit sees that noise


def test_black_and_constant_images_stay_as_they_are(gs):
    ref = R.random_case(1, 12, 16, 4)[1][0]
    ident = gs.colorcorrect.identity_warps(1, 5)[0]
    black = torch.zeros(12, 16, 3)
    out, warps = gs.color_correct(black, ref, return_warps=True)
    assert torch.equal(out, black) and torch.equal(warps, ident)
    const = torch.full((12, 16, 3), 0.5)
    out, warps = gs.color_correct(const, ref, return_warps=True)
    assert torch.isfinite(out).all() and torch.equal(out, const) and torch.equal(warps, ident)
    one = gs.color_correct(torch.full((1, 1, 3), 0.25), torch.full((1, 1, 3), 0.75))
    assert torch.equal(one, torch.full((1, 1, 3), 0.25))
    # one constant channel: that feature set is rank-deficient for every output channel
    img = R.random_case(1, 12, 16, 5)[0][0]
    img[..., 1] = 0.5
    out = gs.color_correct(img, ref)
    assert torch.equal(out, img)


def test_argument_checks_and_detach(gs):
    img, ref = (t[0] for t in R.random_case(1, 5, 7, 6))
    with pytest.raises(ValueError):
        gs.color_correct(img, ref[:4])
    with pytest.raises(ValueError):
        gs.color_correct(img.double(), ref.double())
    with pytest.raises(ValueError):
        gs.color_correct(img.permute(2, 0, 1), ref.permute(2, 0, 1))
    with pytest.raises(ValueError):
        gs.color_correct(img[0], ref[0])
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.colorcorrect.color_correct_hip(img[None], ref[None])
    out = gs.color_correct(img.clone().requires_grad_(True), ref)
    assert not out.requires_grad and torch.equal(out, gs.color_correct(img, ref))
    assert torch.equal(gs.color_correct(img, ref, num_iters=0), img)


# ---- evaluation surface ------------------------------------------------------------------------------------------------
H_, W_ = 24, 32


def _model(gs, **cfg_kw):
    g = torch.Generator().manual_seed(0)
    n = 40
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, **cfg_kw)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.empty(n, 3).uniform_(-5.0, -3.0, generator=g),
                                    torch.randn(n, 4, generator=g), torch.empty(n).uniform_(0.0, 3.0, generator=g),
                                    torch.rand(n, 3, generator=g), torch.randn(n, 3, 3, generator=g) * 0.1, num_cameras=3)


def _scene(gs, model):
    """a stand-in render (one fixed picture per camera) and ground truth = that picture through an affine colour change"""
    pictures = [R.random_case(1, H_, W_, 30 + i)[1][0].clamp(0.05, 0.95) for i in range(3)]

    def render(camera, detach_gaussians=False, return_depth=None):
        return {"rgb": pictures[int(camera.metadata["cam_idx"])]}
    model._render = render
    model._render_batch = lambda cams, dg=False, rd=None: {"rgb": torch.stack([render(c)["rgb"] for c in cams])}
    cams = [gs.Camera(torch.eye(4)[:3], 10.0, 10.0, W_ / 2, H_ / 2, W_, H_, metadata={"cam_idx": i}) for i in range(3)]
    noise = torch.rand(H_, W_, 3, generator=torch.Generator().manual_seed(8)) - 0.5
    images = [(p * torch.tensor([0.8, 0.95, 1.1]) + torch.tensor([0.04, 0.0, -0.03]) + 0.02 * noise).clamp(0, 1)
              for p in pictures]
    return cams, images, pictures


def test_evaluate_reports_the_corrected_metrics_only_when_asked(gs):
    assert gs.SplatfactoDeblurConfig().color_corrected_metrics is False
    model = _model(gs)
    cams, images, pictures = _scene(gs, model)
    plain = gs.training.evaluate(model, cams, images, [0, 1, 2])
    assert set(plain) == {"psnr", "ssim"}
    assert gs.training.evaluate(model, cams, images, [0, 1, 2], color_corrected=False) == plain
    on = gs.training.evaluate(model, cams, images, [0, 1, 2], color_corrected=True)
    assert set(on) == {"psnr", "ssim", "cc_psnr", "cc_ssim"}
    assert on["psnr"] == plain["psnr"] and on["ssim"] == plain["ssim"]
    print(f"psnr {on['psnr']:.2f} -> cc_psnr {on['cc_psnr']:.2f}; ssim {on['ssim']:.4f} -> cc_ssim {on['cc_ssim']:.4f}")
    assert on["cc_psnr"] > on["psnr"] + 3.0 and on["cc_ssim"] > on["ssim"]
    # by hand, from the reference
    want = [gs.training.psnr(R.reference(p, im)[0].float(), im) for p, im in zip(pictures, images)]
    assert on["cc_psnr"] == pytest.approx(sum(want) / 3, abs=1e-3)
    # the batch route makes ONE color_correct call per render batch and reports the same numbers
    calls = []
    real = gs.colorcorrect.color_correct
    gs.colorcorrect.color_correct = lambda *a, **k: (calls.append(tuple(a[0].shape)), real(*a, **k))[1]
    try:
        batched = gs.training.evaluate(model, cams, images, [0, 1, 2], batch_size=2, color_corrected=True)
    finally:
        gs.colorcorrect.color_correct = real
    assert calls == [(2, H_, W_, 3), (1, H_, W_, 3)]
    assert batched == pytest.approx(on, abs=1e-6)
    # the config switch is what None reads
    model_on = _model(gs, color_corrected_metrics=True)
    _scene(gs, model_on)
    assert gs.training.evaluate(model_on, cams, images, [0, 1, 2]) == on
    assert set(gs.training.evaluate(model_on, cams, images, [0], color_corrected=False)) == {"psnr", "ssim"}


def test_old_checkpoint_configs_load_with_the_switch_off(gs):
    d = gs.checkpoint.config_to_dict(gs.SplatfactoDeblurConfig(color_corrected_metrics=True))
    assert d["color_corrected_metrics"] is True
    assert gs.checkpoint.config_from_dict(d).color_corrected_metrics is True
    del d["color_corrected_metrics"]                                     # a file written before the field existed
    assert gs.checkpoint.config_from_dict(d).color_corrected_metrics is False


def test_a_checkpoint_restores_into_a_model_with_the_switch_flipped(gs, tmp_path):
    """the switch only chooses what evaluate() reports; every other config difference still refuses the restore"""
    saved = _model(gs)
    gs.checkpoint.save_checkpoint(tmp_path / "c.pt", saved)
    into = _model(gs, color_corrected_metrics=True)
    with torch.no_grad():
        into.means.add_(1.0)
    gs.checkpoint.load_checkpoint(tmp_path / "c.pt", into=into)
    assert torch.equal(into.means.detach(), saved.means.detach()) and into.config.color_corrected_metrics is True
    with pytest.raises(ValueError, match="config differs"):
        gs.checkpoint.load_checkpoint(tmp_path / "c.pt", into=_model(gs, blur_samples=3))


# ---- C ABI ------------------------------------------------------------------------------------------------------
def _strip(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_new_exports_in_header_definitions_ctypes_table_and_integration_doc(gs):
    from gsdeblur_amd import _lib, _build
    hdr = _strip((ROOT / "include" / "gsdeblur.h").read_text())
    src = _strip(HIP.read_text())
    doc = (ROOT / "INTEGRATION.md").read_text()
    table = {**_lib._SIGS, **_lib._SIGS_LL}
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, hdr)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == nargs, name
        d = re.search(r"GS_EXPORT\s+[\w\s\*]+?\b%s\s*\(([^{};]*?)\)\s*\{" % name, src)
        assert d, f"{name} not defined in colorcorrect.hip"
        assert len(d.group(1).split(",")) == nargs, name
        assert len(table[name]) == nargs and name in _lib.exported_names()
        assert hasattr(_lib.load(), name)
        assert f"`{name}`" in doc, f"{name} missing from INTEGRATION.md"
    assert "colorcorrect.hip" in [s for s, _ in _build.SOURCES]
    # no environment, no allocation, no state, no float atomics in the new file
    for word in ("getenv", "hipMalloc", "hipFree", "static ", "atomicAdd", "atomic_add", "__hip_atomic"):
        assert word not in src, word
    lib = _lib.load()
    assert lib.gs_color_correct_workspace_bytes(0, 1080, 1920) == 0
    one = lib.gs_color_correct_workspace_bytes(1, 1080, 1920)
    assert 0 < one < 4 << 20 and lib.gs_color_correct_workspace_bytes(8, 1080, 1920) == 8 * one
    assert lib.gs_color_correct_workspace_bytes(1, 1, 1) == (30 + 195) * 8
    assert lib.gs_color_correct_workspace_bytes(1, 0, 7) < 0
    # B == 0 is a no-op that touches no pointer; invalid arguments are refused on the host
    assert lib.gs_color_correct(0, 4, 4, None, None, 5, R.EPS, None, None, None, 0, None) == 0
    assert lib.gs_color_correct(1, 4, 4, None, None, 5, R.EPS, None, None, None, 0, None) == 1       # null pointers
    assert lib.gs_color_correct(1, 0, 4, None, None, 5, R.EPS, None, None, None, 0, None) == 1
    assert lib.gs_color_correct(1, 4, 4, None, None, -1, R.EPS, None, None, None, 0, None) == 1
