"""Absgrad densification statistic, host side (no GPU): the per-pair float64 reference anchored to the oracle, the
densification switch, the Python surface and the register budgets of the absgrad backward compositors."""
import inspect
import math
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from absgrad_reference import absgrad_part  # noqa: E402


def _scene(O, n, W, H, seed):
    sc = O.synthetic_scene(n, W, H, seed=seed, scale_mult=6.0)
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 20, sc["ang_vel"] * 10
    return sc


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("S,R", [(1, 1), (3, 2), (5, 1)])
def test_reference_signed_sum_equals_oracle_autograd(oracle, S, R):
    """every part of the frame, gradient conventions 6 (default) and 0 (true derivatives): the helper's signed
    per-Gaussian sum equals xys.grad of autograd through O.rasterize_sorted to 1e-12 of the largest element, and
    abs >= |signed| element-wise.  Part 0 is also checked with a non-zero background (the T_final bg term)."""
    O = oracle
    W, H, n = 128, 96, 3000
    sc = _scene(O, n, W, H, 41)
    cfg = O.RenderConfig(H, W, sc["fx"], sc["fy"], sc["cx"], sc["cy"], blur_samples=S, rs_bands=R, exposure_time=1 / 60,
                         rolling_shutter_time=1 / 30, gamma=1.0, min_rgb_level=0.0)
    q = {k: sc[k].double() for k in ["means", "log_scales", "quats", "opacity_logits", "sh", "viewmat", "lin_vel", "ang_vel"]}
    with torch.no_grad():
        _, _, _, _, parts, _ = O.render(cfg, q["means"], q["log_scales"].exp(), q["quats"],
                                        torch.sigmoid(q["opacity_logits"]), q["sh"], q["viewmat"], q["lin_vel"],
                                        q["ang_vel"], return_parts=True)
    _, _, band = O.subpose_times(cfg.blur_samples, cfg.exposure_time, cfg.rs_bands, cfg.rolling_shutter_time)
    rows = O.band_tile_rows(H, cfg.rs_bands)
    assert len(parts) == S * R
    g = torch.Generator().manual_seed(8)
    bg = torch.tensor([0.3, 0.6, 0.1], dtype=torch.float64)
    worst = 0.0
    for p, (pr, keys, gids, bins, r, rgb, op) in enumerate(parts):
        wc = torch.rand(H, W, 3, generator=g, dtype=torch.float64) - 0.5
        wc[r.fragile] = 0.0
        for up, back in [(O.DEFAULT_GRADS, None), (0, None)] + ([(O.DEFAULT_GRADS, bg)] if p == 0 else []):
            xy = pr.xys.detach().clone().requires_grad_(True)
            rd = O.rasterize_sorted(xy, pr.conics.detach(), rgb.detach(), op.detach(), gids, bins, H, W, back,
                                    tile_rows=rows[band[p]], upstream=up & O.UP_ALPHA_CLAMP)
            (rd.img * wc).sum().backward()
            sgn, ab = absgrad_part(O, pr.xys.detach(), pr.conics.detach(), rgb.detach(), op.detach(), gids, bins, H, W, wc,
                                   tile_rows=rows[band[p]], upstream=up, background=back)
            err = float((sgn - xy.grad).abs().max() / xy.grad.abs().max())
            worst = max(worst, err)
            assert err <= 1e-12, (p, up, err)
            assert bool((ab >= sgn.abs() * (1 - 1e-12)).all())
            assert float(ab.max()) > 0
    print(f"S={S} R={R}: signed sum vs autograd, worst relative error {worst:.2e}")


# ---- densification switch ------------------------------------------------------------------------------------------
def _model(gs, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.full((n, 3), math.log(0.005)),
                                    torch.randn(n, 4, generator=g), torch.full((n,), 2.0), torch.rand(n, 3, generator=g),
                                    torch.zeros(n, 3, 3))


@pytest.mark.parametrize("absgrad", [False, True])
def test_cancelled_gradient_densifies_only_with_absgrad(gs, absgrad):
    """Gaussians 0 (big) and 1 (small): signed sum exactly zero, large absgrad -> split / duplicated with the switch, left
    alone without it"""
    n = 6
    model = _model(gs, n)
    opts = gs.training.make_optimizers(model)
    with torch.no_grad():
        model.scales[0] = math.log(0.05)
    cfg = gs.densify.DensifyConfig(n_split_samples=2, absgrad=absgrad)
    st = gs.densify.DensifyState(n, "cpu", absgrad=absgrad)
    radii = torch.full((2, n), 3, dtype=torch.int32)
    xy = torch.zeros(n, 2)
    xa = torch.zeros(n, 2)
    xa[0] = torch.tensor([3.0, 4.0])
    xa[1] = torch.tensor([0.6, 0.8])
    st.after_backward(radii, xy, 100, 100, xy_absgrad=xa)
    assert st.xys_grad_norm.tolist() == pytest.approx([5.0, 1.0, 0, 0, 0, 0] if absgrad else [0.0] * 6)
    assert st.vis_counts.tolist() == [1.0] * n and st.max_2Dsize.tolist() == pytest.approx([0.03] * n)
    res = gs.densify.refine(model, opts, st, step=600, cfg=cfg)
    if absgrad:
        assert (res["split"], res["duplicated"], res["after"]) == (1, 1, n - 1 + 2 + 1)
        assert st.absgrad                                   # the fresh state keeps the switch
    else:
        assert (res["split"], res["duplicated"], res["after"]) == (0, 0, n)


def test_absgrad_batch_equals_single_calls_and_missing_tensor_raises(gs):
    B, P, n = 3, 2, 7
    g = torch.Generator().manual_seed(3)
    radii = torch.randint(0, 4, (B, P, n), generator=g, dtype=torch.int32)
    xy = torch.randn(B, n, 2, generator=g)
    xa = torch.rand(B, n, 2, generator=g)
    a = gs.densify.DensifyState(n, "cpu", absgrad=True)
    a.after_backward(radii, xy, 64, 48, xy_absgrad=xa)
    b = gs.densify.DensifyState(n, "cpu", absgrad=True)
    for k in range(B):
        b.after_backward(radii[k], xy[k], 64, 48, xy_absgrad=xa[k])
    c = gs.densify.DensifyState(n, "cpu", absgrad=True)
    c.after_backward(list(radii), None, 64, 48, xy_absgrad=list(xa))          # lists (mixed-intrinsics groups)
    for s in (b, c):
        assert torch.equal(a.xys_grad_norm, s.xys_grad_norm) and torch.equal(a.vis_counts, s.vis_counts)
        assert torch.equal(a.max_2Dsize, s.max_2Dsize)
    # the signed state ignores the extra tensor
    d, e = gs.densify.DensifyState(n, "cpu"), gs.densify.DensifyState(n, "cpu")
    d.after_backward(radii, xy, 64, 48, xy_absgrad=xa)
    e.after_backward(radii, xy, 64, 48)
    assert torch.equal(d.xys_grad_norm, e.xys_grad_norm) and not torch.equal(d.xys_grad_norm, a.xys_grad_norm)
    with pytest.raises(ValueError, match="xy_absgrad"):
        gs.densify.DensifyState(n, "cpu", absgrad=True).after_backward(radii[0], xy[0], 64, 48)


def test_step_callback_needs_the_absgrad_tensor(gs):
    model = _model(gs, 5)
    opts = gs.training.make_optimizers(model)
    cfg = gs.densify.DensifyConfig(absgrad=True)
    st = gs.densify.DensifyState(5, "cpu", absgrad=True)
    model.radii = torch.ones(1, 5, dtype=torch.int32)
    model.xy_grad = torch.zeros(5, 2)
    model.last_size = (64, 48)
    with pytest.raises(ValueError, match="densify_absgrad"):
        gs.densify.step_callback(model, opts, st, 1, cfg)
    model.xy_absgrad = torch.ones(5, 2)
    gs.densify.step_callback(model, opts, st, 1, cfg)
    assert st.xys_grad_norm.tolist() == pytest.approx([math.sqrt(2.0)] * 5)
    with pytest.raises(ValueError, match="disagree"):
        gs.densify.step_callback(model, opts, gs.densify.DensifyState(5, "cpu"), 1, cfg)


# ---- Python surface ------------------------------------------------------------------------------------------------
def test_entry_points_take_xy_absgrad_out(gs):
    from gsdeblur_amd import ops
    from gsdeblur_amd.step import render_step
    for fn in (ops.render_subposes, ops.render_combined, ops.render_batch, render_step):
        p = inspect.signature(fn).parameters
        assert "xy_absgrad_out" in p and p["xy_absgrad_out"].default is None, fn.__name__
    assert gs.SplatfactoDeblurConfig().densify_absgrad is False
    assert gs.densify.DensifyConfig().absgrad is False and gs.densify.DensifyConfig().densify_grad_thresh == 0.0008


def test_pixel_velocity_model_refuses_absgrad_before_any_device_work(gs):
    """CPU tensors: the ValueError must come before anything touches the library or a device"""
    from gsdeblur_amd import ops
    from gsdeblur_amd.step import render_step
    n, H, W, S = 8, 32, 32, 3
    g = torch.Generator().manual_seed(0)
    means, scales, quats = torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g), torch.randn(n, 4, generator=g)
    opac, sh = torch.rand(n, generator=g), torch.rand(n, 16, 3, generator=g)
    V, lin, ang = torch.eye(4), torch.zeros(3), torch.zeros(3)
    times = torch.linspace(-0.01, 0.01, S)
    out = torch.empty(n, 2)
    for fn, kw in ((ops.render_subposes, {}), (ops.render_combined, dict(gamma=2.2))):
        with pytest.raises(ValueError, match="pixel-velocity"):
            fn(means, scales, quats, opac, sh, V, None, S, 1, 30.0, 30.0, 16.0, 16.0, H, W, lin_vel=lin, ang_vel=ang,
               times=times, xy_absgrad_out=out, **kw)
    with pytest.raises(ValueError, match="pixel-velocity"):
        ops.render_batch(means, scales, quats, opac, sh, V.expand(2, S, 4, 4), None, S, 1, 30.0, 30.0, 16.0, 16.0, H, W,
                         times=times, xy_absgrad_out=torch.empty(2, n, 2))
    with pytest.raises(ValueError, match="pixel-velocity"):
        render_step(means, scales, quats, opac, sh, V, lin, ang, times, None, S, 1, 30.0, 30.0, 16.0, 16.0, H, W,
                    torch.zeros(H, W, 3), motion_model="pixel_velocity", xy_absgrad_out=out)


def test_twin_backend_raises_on_absgrad(gs, monkeypatch):
    """the Python frame backend of the tests has no absgrad compositor: refused before any launch (CPU tensors)"""
    from gsdeblur_amd import ops
    monkeypatch.setattr(ops, "NATIVE_FRAME", 0)
    assert ops.frame_backend is not None and not ops.frame_backend.native_ok()
    n, H, W = 8, 32, 32
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="frame backend"):
        ops.render_subposes(torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g),
                            torch.randn(n, 4, generator=g), torch.rand(n, generator=g), torch.rand(n, 16, 3, generator=g),
                            torch.eye(4)[None], None, 1, 1, 30.0, 30.0, 16.0, 16.0, H, W,
                            xy_absgrad_out=torch.empty(n, 2))


# ---- register budgets of the four absgrad instantiations ----------------------------------------------------------------
# What the build produces (gfx950, the library's flags), rounded up to the 8-register allocation granule: the state-less
# rgb forms 80, with reverse-traversal state 87 -> 88, the depth forms 85 -> 88 and 91 -> 96.  All inside the 96 that
# five waves per SIMD allow (the launch bound of the default kernels, untouched), none spills a VGPR.
# raster_bwd_sload_kernel<STATE, OUT, DEPTH, ABSGRAD, CAMS>: the ABSGRAD = true instantiations
BUDGET = {
    "raster_bwd_sload_kernel<false, 1, false, true, false>": 80,
    "raster_bwd_sload_kernel<true, 1, false, true, false>": 88,
    "raster_bwd_sload_kernel<false, 1, false, true, true>": 80,
    "raster_bwd_sload_kernel<true, 1, false, true, true>": 88,
    "raster_bwd_sload_kernel<false, 1, true, true, false>": 88,
    "raster_bwd_sload_kernel<true, 1, true, true, false>": 96,
    "raster_bwd_sload_kernel<false, 1, true, true, true>": 88,
    "raster_bwd_sload_kernel<true, 1, true, true, true>": 96,
}
# LDS per block of four waves: 4 x 4 entries x (11 | 12) rows x 36 floats; five blocks per CU must fit into 160 KB
LDS_BYTES = {False: 4 * 4 * 11 * 36 * 4, True: 4 * 4 * 12 * 36 * 4}


@pytest.mark.timeout(900)
def test_absgrad_kernels_stay_inside_their_register_budgets(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gsd_build", ROOT / "3dgs-deblur_amd" / "_build.py")
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    hipcc = B._hipcc()
    if shutil.which(hipcc) is None or shutil.which("c++filt") is None:
        pytest.skip("no hipcc / c++filt on this host")
    f = tmp_path / "raster_bwd.s"
    subprocess.check_call([hipcc, *B.COMMON, *dict(B.SOURCES)["raster_bwd.hip"], "-S", "--cuda-device-only",
                           str(B.CSRC / "raster_bwd.hip"), "-o", str(f)], stderr=subprocess.DEVNULL)
    meta = {}
    for blk in f.read_text().split("- .agpr_count")[1:]:
        def num(key):
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (num("vgpr_count"), num("vgpr_spill_count"),
                                                              num("group_segment_fixed_size"),
                                                              num("private_segment_fixed_size"))
    names = list(meta)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    seen = {d.split("(")[0].replace("void gs::", ""): meta[m] for m, d in zip(names, dem)}
    for frag, max_vgpr in BUDGET.items():
        assert frag in seen, (frag, sorted(seen))
        vgpr, spill, lds, scratch = seen[frag]
        print(f"{frag}: {vgpr} VGPRs (budget {max_vgpr}), {spill} spilled, {lds} B LDS, {scratch} B scratch")
        assert vgpr <= max_vgpr <= 96, (frag, vgpr)
        assert spill == 0 and scratch == 0, (frag, spill, scratch)
        assert lds == LDS_BYTES[frag.split(", ")[2] == "true"], (frag, lds)      # DEPTH: the third template argument
        assert 5 * lds <= 160 * 1024
