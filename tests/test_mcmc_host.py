"""3DGS-MCMC on the CPU: csrc/mcmc_math.h compiled with g++ against the float64 reference (tests/mcmc_reference.py) —
Philox known answers, normals, noise displacement, relocation —, the strategy logic of mcmc.py on CPU tensors with
torch Adam, the two regularisers on train_step's CPU route, a world-2 gloo run, and the C-ABI entries."""
import ctypes
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mcmc_reference as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "mcmc_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libmcmc_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "mcmc_math.h"
NEW_EXPORTS = {"gs_mcmc_inject_noise": 11, "gs_mcmc_relocation": 7}


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def mh():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{HDR.parent}", str(SRC), "-o",
                               str(LIB)])
    return ctypes.CDLL(str(LIB))


# ---- Philox + normals ---------------------------------------------------------------------------------------------
KNOWN = (
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def _words(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox4x32_10_known_answers(mh, counter, key, want):
    """Random123's known-answer vectors, in the header's host build and in the Python reference"""
    c, k = np.array(_words(counter), np.uint32), np.array(_words(key), np.uint32)
    out = np.zeros(4, np.uint32)
    mh.mh_philox(P(c), P(k), P(out))
    assert [int(x) for x in out] == _words(want)
    assert R.philox4x32_10(_words(counter), _words(key)) == _words(want)


def test_row_words_use_counter_row_0_step_and_key_seed(mh):
    seed, step = 0x0123456789ABCDEF, 0x0000000300000007
    n = 5
    w = np.zeros((n, 4), np.uint32)
    mh.mh_row_words(n, ctypes.c_ulonglong(seed), ctypes.c_ulonglong(step), P(w))
    for r in range(n):
        assert [int(x) for x in w[r]] == R.philox4x32_10([r, 0, 7, 3], [0x89ABCDEF, 0x01234567])
        assert [int(x) for x in w[r]] == R.row_words(r, seed, step)


def test_normals_against_float64_and_their_range(mh):
    """from the same fp32 u: the product 2 pi u rounds once more (angle error up to 4e-7), the radius is at most 6.76,
    cosf / sinf / logf / sqrtf add a few ulps -> below 3e-6; 1e-5 absolute is the bar.  The extreme words give the
    extreme values: u = 2^-33 (radius 6.76) and u = 1 (radius 0)."""
    n = 50_000
    w = np.zeros((n, 4), np.uint32)
    mh.mh_row_words(n, ctypes.c_ulonglong(3), ctypes.c_ulonglong(11), P(w))
    w[0] = (0, 0, 0xFFFFFFFF, 0x80000000)
    z = np.zeros((n, 3), np.float32)
    mh.mh_normals(n, P(w), P(z))
    ref = R.normals_from_words(torch.from_numpy(w.astype(np.int64)))
    assert np.isfinite(z).all()
    assert float((torch.from_numpy(z).double() - ref).abs().max()) < 1e-5
    assert abs(z[0, 0] - math.sqrt(-2 * math.log(2.0 ** -33))) < 1e-5 and abs(z[0, 2]) < 1e-5
    assert np.abs(z).max() <= 6.8
    assert abs(z.mean()) < 5 / math.sqrt(z.size) and abs(z.var() - 1) < 5 * math.sqrt(2 / z.size)


# ---- relocation ---------------------------------------------------------------------------------------------------
def relocation_grid():
    """every n in 1 .. 51 x o in {0.005, 0.01, 0.1, 0.5, 0.9, 0.999}, scales spread over three decades"""
    os_ = (0.005, 0.01, 0.1, 0.5, 0.9, 0.999)
    n = torch.arange(1, 52, dtype=torch.int32).repeat_interleave(len(os_))
    o = torch.tensor(os_, dtype=torch.float32).repeat(51)
    g = torch.Generator().manual_seed(5)
    s = torch.exp(torch.empty(n.numel(), 3).uniform_(math.log(1e-3), math.log(1.0), generator=g))
    return o, s, n


def assert_relocation_close(new_o, new_s, o, s, n, tol=1e-6):
    ro, rs = R.relocation(o, s, n)
    eo = ((new_o.double() - ro).abs() / ro.abs()).max().item()
    es = ((new_s.double() - rs).abs() / rs.abs()).max().item()
    print(f"relocation: max rel err o' {eo:.2e}, s' {es:.2e} over {o.numel()} rows")
    assert eo <= tol and es <= tol, (eo, es)


def _mh_relocation(mh, o, s, n):
    on, sn, nn = (np.ascontiguousarray(t.numpy()) for t in (o, s, n))
    new_o, new_s = np.zeros_like(on), np.zeros_like(sn)
    mh.mh_relocation(len(on), P(on), P(sn), P(nn), P(new_o), P(new_s))
    return torch.from_numpy(new_o), torch.from_numpy(new_s)


def test_relocation_against_float64_on_the_grid(mh):
    o, s, n = relocation_grid()
    new_o, new_s = _mh_relocation(mh, o, s, n)
    assert_relocation_close(new_o, new_s, o, s, n)
    one = n == 1                                           # one copy: nothing changes
    assert ((new_o[one] - o[one]).abs() <= 1e-6 * o[one]).all()
    assert ((new_s[one] - s[one]).abs() <= 1e-6 * s[one]).all()
    # the correction shrinks: more copies, lower opacity and smaller scale each
    assert (new_o[~one] < o[~one]).all() and (new_s[~one] < s[~one]).all()


def test_relocation_clamps_the_ratio_to_51(mh):
    o, s, n = relocation_grid()
    at51 = n == 51
    a = _mh_relocation(mh, o[at51], s[at51], n[at51])
    for big in (52, 100, 2 ** 30):
        b = _mh_relocation(mh, o[at51], s[at51], torch.full_like(n[at51], big))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    z = _mh_relocation(mh, o[at51], s[at51], torch.zeros_like(n[at51]))      # below 1: one copy
    assert torch.allclose(z[0], o[at51], rtol=1e-6)


def test_torch_relocation_matches_the_reference(gs):
    o, s, n = relocation_grid()
    new_o, new_s = gs.mcmc.relocation_torch(o, s, n)
    assert_relocation_close(new_o, new_s, o, s, n)


# ---- noise displacement ---------------------------------------------------------------------------------------------
def noise_case(n, seed=0):
    """unnormalised quaternions, scale ratios up to 100 inside a Gaussian, logits spread so that the opacity covers
    1e-4 .. 0.999 (dense around the gate's 0.005)"""
    g = torch.Generator().manual_seed(seed)
    quats = torch.randn(n, 4, generator=g) * torch.empty(n, 1).uniform_(0.1, 5.0, generator=g)
    base = torch.empty(n, 1).uniform_(math.log(0.01), math.log(0.2), generator=g)
    log_scales = base + torch.empty(n, 3).uniform_(math.log(0.1), math.log(10.0), generator=g)
    o = torch.exp(torch.empty(n).uniform_(math.log(1e-4), math.log(0.999), generator=g))
    logits = torch.log(o / (1 - o)).float()
    z = torch.randn(n, 3, generator=g)
    means = torch.randn(n, 3, generator=g)
    return means, log_scales.float(), quats.float(), logits, z


def assert_delta_close(delta, ref):
    """the project's gradient bar: per element |d - ref| <= 1e-4 |ref| + 1e-5 max|ref|"""
    err = (delta.double() - ref).abs()
    bound = 1e-4 * ref.abs() + 1e-5 * ref.abs().max()
    worst = (err / bound).max().item()
    print(f"noise displacement: worst error / bound = {worst:.3f}, max|ref| = {ref.abs().max().item():.3e}")
    assert worst <= 1.0, worst


def test_noise_displacement_against_float64(mh):
    n = 20_000
    _, ls, q, l, z = noise_case(n)
    scaler = 5e5 * 1.6e-4
    d = np.zeros((n, 3), np.float32)
    mh.mh_noise_delta(n, P(ls.numpy()), P(q.numpy()), P(l.numpy()), P(z.numpy()), ctypes.c_float(scaler), P(d))
    ref = R.noise_delta(ls, q, l, z, scaler)
    o = torch.sigmoid(l.double())
    assert o.min() < 2e-4 and o.max() > 0.99 and ((o > 0.003) & (o < 0.008)).sum() > 100
    assert ref.abs().max() > 0 and (ref[o > 0.95].abs().max() < 1e-30)      # opaque Gaussians do not move
    assert_delta_close(torch.from_numpy(d), ref)


def test_torch_noise_matches_the_reference_and_is_seeded_by_seed_and_step(gs):
    n = 2000
    means, ls, q, l, z = noise_case(n, seed=2)
    scaler = 80.0
    m = means.clone()
    gs.mcmc.inject_noise_torch(m, ls, q, l, scaler, 0, 0, noise_in=z)
    ref = R.noise_delta(ls, q, l, z, scaler)
    assert ((m - means).double() - ref).abs().max() <= 1e-4 * ref.abs().max()
    outs = []
    for seed, step in ((1, 5), (1, 5), (1, 6), (2, 5)):
        m, used = means.clone(), torch.empty(n, 3)
        gs.mcmc.inject_noise_torch(m, ls, q, l, scaler, seed, step, noise_out=used)
        outs.append((m, used))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][1], outs[2][1]) and not torch.equal(outs[0][1], outs[3][1])


# ---- strategy logic on CPU tensors -----------------------------------------------------------------------------------
def _model(gs, n, seed=0, **cfg_kw):
    g = torch.Generator().manual_seed(seed)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, **cfg_kw)
    opac = torch.empty(n).uniform_(0.0, 3.0, generator=g)             # sigmoid: 0.5 .. 0.95
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g),
                                    torch.empty(n, 3).uniform_(-5.0, -3.0, generator=g),
                                    torch.randn(n, 4, generator=g), opac, torch.rand(n, 3, generator=g),
                                    torch.randn(n, 3, 3, generator=g) * 0.1)


def _prime_adam(gs, model, **kw):
    opts = gs.training.make_optimizers(model, **kw)
    g = torch.Generator().manual_seed(9)
    for p in model.gauss_params().values():
        p.grad = torch.randn(p.shape, generator=g)
    for o in opts.values():
        o.step(torch.ones(model.num_points, dtype=torch.bool)) if getattr(o, "selective", False) else o.step()
    return opts


def test_config_defaults(gs):
    c = gs.mcmc.MCMCConfig()
    assert (c.cap_max, c.noise_lr, c.refine_start_iter, c.refine_stop_iter, c.refine_every, c.min_opacity,
            c.grow_factor, c.seed) == (1_000_000, 5e5, 500, 25_000, 100, 0.005, 1.25, 0)
    m = gs.SplatfactoDeblurConfig()
    assert m.opacity_reg == 0.0 and m.scale_reg == 0.0


@pytest.mark.parametrize("optimizer", ["adam", "selective_adam"])
def test_relocate_moves_dead_rows_onto_live_ones_and_resets_the_sampled_moments(gs, optimizer):
    n = 200
    model = _model(gs, n)
    opts = _prime_adam(gs, model, optimizer=optimizer)
    cfg = gs.mcmc.MCMCConfig()
    dead = torch.zeros(n, dtype=torch.bool)
    dead[::7] = True
    with torch.no_grad():
        model.opacities[dead] = -8.0                                   # sigmoid = 3e-4 <= min_opacity
    old = {k: p.detach().clone() for k, p in model.gauss_params().items()}
    old_st = {k: {s: opts[k].state[p][s].clone() for s in ("exp_avg", "exp_avg_sq")}
              for k, p in model.gauss_params().items()}
    res = gs.mcmc.relocate(model, opts, step=600, cfg=cfg)
    assert res == {"relocated": int(dead.sum()), "dead": int(dead.sum()), "before": n, "after": n}
    assert model.num_points == n
    assert not (torch.sigmoid(model.opacities.detach()) <= cfg.min_opacity).any()        # no dead row is left
    # every dead row now equals a live source row in EVERY parameter; the sources are the rows whose opacity changed
    changed = (model.opacities.detach() != old["opacities"]).reshape(-1) & ~dead
    assert changed.any()
    src_ids = changed.nonzero().reshape(-1)
    for d in dead.nonzero().reshape(-1).tolist():
        hit = [int(s) for s in src_ids if torch.equal(model.means[d], model.means[s])]
        assert len(hit) == 1, d
        for k, p in model.gauss_params().items():
            assert torch.equal(p[d], p[hit[0]]), (k, d)
    # sources: corrected opacity and scale (lower, smaller), everything else as before
    assert (model.opacities.detach()[changed] < old["opacities"][changed]).all()
    assert (model.scales.detach()[changed] < old["scales"][changed]).all()
    for k in ("means", "quats", "features_dc", "features_rest"):
        assert torch.equal(model.gauss_params()[k].detach()[~dead], old[k][~dead])
    untouched = ~dead & ~changed
    for k, p in model.gauss_params().items():
        assert torch.equal(p.detach()[untouched], old[k][untouched])
        assert opts[k].param_groups[0]["params"][0] is p
        for s in ("exp_avg", "exp_avg_sq"):
            st = opts[k].state[p][s]
            assert float(st[changed].abs().sum()) == 0                 # zero exactly on the sampled rows
            assert torch.equal(st[~changed], old_st[k][s][~changed])   # ... and unchanged elsewhere (dead rows too)
            assert float(old_st[k][s][changed].abs().sum()) > 0


def test_relocate_applies_the_reference_correction_for_the_drawn_multiplicity(gs):
    n = 60
    model = _model(gs, n, seed=4)
    opts = _prime_adam(gs, model)
    with torch.no_grad():
        model.opacities[:40] = -9.0
    old_o = torch.sigmoid(model.opacities.detach().reshape(-1))
    old_s = torch.exp(model.scales.detach())
    gs.mcmc.relocate(model, opts, step=700, cfg=gs.mcmc.MCMCConfig())
    for s in range(40, n):
        copies = sum(1 for d in range(40) if torch.equal(model.means[d], model.means[s]))
        ro, rs = R.relocation(old_o[s:s + 1], old_s[s:s + 1], torch.tensor([copies + 1]))
        assert torch.allclose(torch.sigmoid(model.opacities.detach()[s]).double(), ro, rtol=1e-5)
        assert torch.allclose(torch.exp(model.scales.detach()[s]).double(), rs[0], rtol=1e-5)


def test_relocate_without_dead_rows_is_a_no_op(gs):
    model = _model(gs, 30)
    opts = _prime_adam(gs, model)
    old = {k: p.detach().clone() for k, p in model.gauss_params().items()}
    assert gs.mcmc.relocate(model, opts, 600, gs.mcmc.MCMCConfig())["relocated"] == 0
    for k, p in model.gauss_params().items():
        assert torch.equal(p.detach(), old[k])


def test_add_new_grows_geometrically_to_the_cap_with_zero_moments(gs):
    n = 100
    model = _model(gs, n, seed=1)
    opts = _prime_adam(gs, model)
    cfg = gs.mcmc.MCMCConfig(cap_max=180)
    sizes = []
    for step in (600, 700, 800, 900):
        N0 = model.num_points
        old = {k: p.detach().clone() for k, p in model.gauss_params().items()}
        old_m = {k: opts[k].state[p]["exp_avg"].clone() for k, p in model.gauss_params().items()}
        res = gs.mcmc.add_new(model, opts, step, cfg)
        N1 = model.num_points
        assert N1 == min(cfg.cap_max, int(1.25 * N0)) and res == {"added": N1 - N0, "before": N0, "after": N1}
        sizes.append(N1)
        for k, p in model.gauss_params().items():
            assert p.shape[0] == N1 and p.requires_grad and opts[k].param_groups[0]["params"][0] is p
            st = opts[k].state[p]
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
            assert torch.equal(st["exp_avg"][:N0], old_m[k])                     # old rows keep their moments
            assert float(st["exp_avg"][N0:].abs().sum()) == 0 and float(st["exp_avg_sq"][N0:].abs().sum()) == 0
        if N1 > N0:
            # an appended row is a copy of an old row AFTER its correction
            for r in range(N0, N1):
                src = [s for s in range(N0) if torch.equal(model.means[r], old["means"][s])]
                # (several candidates when the source is itself an earlier copy: identical rows drawn equally often stay identical)
                src = [s for s in src if all(torch.equal(p[r], p[s]) for p in model.gauss_params().values())]
                assert src, r
                assert any(model.opacities[s] < old["opacities"][s] for s in src), r
    assert sizes == [125, 156, 180, 180]
    for p in model.gauss_params().values():                                      # the optimizers still step
        p.grad = torch.ones_like(p)
    for o in opts.values():
        o.step()


def test_step_callback_schedule_and_noise_every_step(gs, monkeypatch):
    cfg = gs.mcmc.MCMCConfig(cap_max=64, refine_start_iter=10, refine_stop_iter=40, refine_every=5)
    model = _model(gs, 32)
    with torch.no_grad():
        model.opacities.fill_(-4.0)                       # o = 0.018: alive, and the gate lets the noise through
    opts = _prime_adam(gs, model)
    notified = []
    monkeypatch.setattr(gs.dp, "notify_regime_change", lambda: notified.append(1))
    refined, sizes = [], []
    for step in range(1, 51):
        before = model.means.detach().clone()
        n0 = model.num_points
        r = gs.mcmc.step_callback(model, opts, step, cfg)
        if r is not None:
            refined.append(step)
            assert r["before"] == n0 and r["after"] == model.num_points
        assert not torch.equal(model.means.detach()[:n0], before)                # noise on EVERY step
        sizes.append(model.num_points)
    assert refined == [15, 20, 25, 30, 35]                # start < step < stop, step % 5 == 0
    assert len(notified) == len(refined)
    assert sizes == sorted(sizes) and max(sizes) == 64 and sizes[13] == 32 and sizes[14] == 40


def test_strategy_is_deterministic_in_seed_and_step(gs):
    def run(seed, step):
        model = _model(gs, 80, seed=3)
        with torch.no_grad():
            model.opacities[::5] = -9.0
            model.opacities[1::5] = -4.0
        opts = _prime_adam(gs, model)
        cfg = gs.mcmc.MCMCConfig(cap_max=1000, refine_start_iter=0, refine_every=1, seed=seed)
        gs.mcmc.step_callback(model, opts, step, cfg)
        return torch.cat([p.detach().reshape(-1) for p in model.gauss_params().values()])
    a, b, c, d = run(0, 7), run(0, 7), run(0, 8), run(1, 7)
    assert torch.equal(a, b)
    assert a.shape == c.shape == d.shape and not torch.equal(a, c) and not torch.equal(a, d)


def test_inject_noise_scales_with_the_means_learning_rate(gs):
    model = _model(gs, 50, seed=6)
    with torch.no_grad():
        model.opacities.fill_(-5.0)
    opts = _prime_adam(gs, model)
    cfg = gs.mcmc.MCMCConfig(noise_lr=1e4)
    m0 = model.means.detach().clone()
    gs.mcmc.inject_noise(model, opts, 3, cfg)
    d1 = model.means.detach() - m0
    g = gs.mcmc._noise_generator(torch.device("cpu"), cfg.seed, 3)
    z = torch.randn(50, 3, generator=g)
    ref = R.noise_delta(model.scales.detach(), model.quats.detach(), model.opacities.detach(), z,
                        1e4 * opts["means"].param_groups[0]["lr"])
    assert (d1.double() - ref).abs().max() <= 1e-4 * ref.abs().max() + 1e-7 * m0.abs().max()
    opts["means"].param_groups[0]["lr"] *= 0.5
    model.means.data.copy_(m0)
    gs.mcmc.inject_noise(model, opts, 3, cfg)
    d2 = model.means.detach() - m0
    assert torch.allclose(d2, 0.5 * d1, rtol=1e-3, atol=1e-7 * float(m0.abs().max()))


# ---- the regularisers on train_step's CPU route --------------------------------------------------------------------
def _fake_render(gs, model, H=12, W=12):
    def fake_outputs(camera):
        n = model.num_points
        model.radii = torch.ones(1, n, dtype=torch.int32)
        col = model.features_dc.mean(0) + 0.01 * model.means.sum() + 0.01 * model.scales.sum() + \
            0.01 * model.opacities.sum() + 0.01 * model.quats.sum() + 0.01 * model.features_rest.sum()
        return {"rgb": (0.1 * col)[None, None, :].expand(H, W, 3)}
    model.get_outputs = fake_outputs
    cam = gs.Camera(torch.eye(4)[:3], 10.0, 10.0, 6.0, 6.0, W, H, metadata={"cam_idx": 0})
    return cam, torch.full((H, W, 3), 0.4)


def _step_grads(gs, model, **kw):
    cam, gt = _fake_render(gs, model)
    opts = gs.training.make_optimizers(model)
    start = {k: p.detach().clone() for k, p in model.gauss_params().items()}
    h = gs.training.train_step(model, opts, cam, gt, **kw)
    return h["loss"], {k: p.grad.clone() for k, p in model.gauss_params().items()}, start, cam, gt


def test_regularisers_at_zero_leave_the_step_unchanged(gs):
    """the default config's loss and gradients are those of the image loss alone (what train_step computed before the
    fields existed), bit for bit — on the single-camera and the batch route"""
    for batch in (False, True):
        model = _model(gs, 40, seed=8)
        assert model.config.opacity_reg == 0.0 and model.config.scale_reg == 0.0
        cam, gt = _fake_render(gs, model)
        opts = gs.training.make_optimizers(model)
        twin = _model(gs, 40, seed=8)
        tcam, _ = _fake_render(gs, twin)
        twin.train()
        ref_loss = gs.training.image_loss_torch(twin.get_outputs(tcam)["rgb"], gt, 0.2)
        ref_loss.backward()
        if batch:
            model.get_outputs_batch = lambda cams, m=model, **kw: {"rgb": [m.get_outputs(c)["rgb"] for c in cams]}
            h = gs.training.train_step(model, opts, [cam], [gt])
        else:
            h = gs.training.train_step(model, opts, cam, gt)
        assert h["loss"] == float(ref_loss.detach().float())
        for k, p in model.gauss_params().items():
            assert torch.equal(p.grad, twin.gauss_params()[k].grad), k


def test_regularisers_match_autograd_of_the_formula(gs):
    base_loss, base_g, _, _, _ = _step_grads(gs, _model(gs, 40, seed=8))
    loss, g, start, _, _ = _step_grads(gs, _model(gs, 40, seed=8, opacity_reg=0.01, scale_reg=0.01))
    o = start["opacities"].double().requires_grad_(True)
    s = start["scales"].double().requires_grad_(True)
    reg = 0.01 * torch.sigmoid(o).mean() + 0.01 * torch.exp(s).mean()
    reg.backward()
    assert loss == pytest.approx(base_loss + float(reg.detach()), rel=1e-6)
    assert torch.allclose((g["opacities"] - base_g["opacities"]).double(), o.grad, rtol=1e-4, atol=1e-9)
    assert torch.allclose((g["scales"] - base_g["scales"]).double(), s.grad, rtol=1e-4, atol=1e-9)
    assert float(o.grad.abs().min()) > 0 and float(s.grad.abs().min()) > 0       # every row gets a gradient
    for k in ("means", "quats", "features_dc", "features_rest"):
        assert torch.equal(g[k], base_g[k])
    # one at a time
    _, g_o, _, _, _ = _step_grads(gs, _model(gs, 40, seed=8, opacity_reg=0.01))
    assert torch.equal(g_o["scales"], base_g["scales"]) and not torch.equal(g_o["opacities"], base_g["opacities"])


def test_train_scene_accepts_an_mcmc_config_and_collects_no_statistic(gs, monkeypatch):
    """the CPU route of train_scene with a stand-in render: N follows the schedule up to the cap, the optimizer state
    tracks it, and no densification statistic is switched on"""
    model = _model(gs, 40, seed=2, opacity_reg=0.01, scale_reg=0.01)
    cam, gt = _fake_render(gs, model)

    class Scene:
        train_indices = [0]
        eval_indices = [0]
        cameras = [cam]
    monkeypatch.setattr(gs.training, "evaluate", lambda *a, **k: {"psnr": 0.0, "ssim": 0.0})
    seen = []
    real = gs.mcmc.step_callback

    def spy(m, o, step, cfg, group=None):
        r = real(m, o, step, cfg, group)
        seen.append(m.num_points)
        for k, p in m.gauss_params().items():
            st = o[k].state[p]
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        return r
    monkeypatch.setattr(gs.mcmc, "step_callback", spy)
    cfg = gs.mcmc.MCMCConfig(cap_max=70, refine_start_iter=2, refine_stop_iter=100, refine_every=3)
    gs.training.train_scene(model, Scene, [gt], 12, densify=cfg)
    assert len(seen) == 12 and seen == sorted(seen) and seen[-1] == 70 and seen[1] == 40 and seen[2] == 50
    assert model.collect_densify_stats is False and model.xy_grad is None


# ---- data parallel ------------------------------------------------------------------------------------------------
def _mcmc_worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import gsdeblur_amd as gs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _model(gs, 60, seed=7)                      # replicated Gaussians
    with torch.no_grad():
        model.opacities[::4] = -9.0
        model.opacities[1::4] = -4.5
    opts = _prime_adam(gs, model)
    cfg = gs.mcmc.MCMCConfig(cap_max=100, refine_start_iter=0, refine_every=1)
    res = None
    for step in (1, 2, 3):
        res = gs.mcmc.step_callback(model, opts, step, cfg)
    flat = torch.cat([p.detach().reshape(-1) for p in model.gauss_params().values()] +
                     [opts[k].state[p][s].reshape(-1) for k, p in model.gauss_params().items()
                      for s in ("exp_avg", "exp_avg_sq")])
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([flat.numel()]))
    same = all(int(s) == flat.numel() for s in sizes)
    if same:
        other = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(other, flat)
        same = all(torch.equal(o, flat) for o in other)
    q.put((rank, same, model.num_points, res["after"]))
    dist.destroy_process_group()


def test_mcmc_world2_gloo_ranks_stay_identical():
    """relocate + add + noise decide from the replicated parameters and (seed, step) alone: replicas stay bit-identical"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41200 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_mcmc_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True, 100, 100), (1, True, 100, 100)]


# ---- C ABI ------------------------------------------------------------------------------------------------------
def _strip(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_new_exports_in_header_definitions_ctypes_table_and_integration_doc(gs):
    from gsdeblur_amd import _lib, _build
    hdr = _strip((ROOT / "include" / "gsdeblur.h").read_text())
    src = _strip((ROOT / "3dgs-deblur_amd" / "csrc" / "mcmc.hip").read_text())
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, hdr)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == nargs, name
        d = re.search(r"GS_EXPORT\s+[\w\s\*]+?\b%s\s*\(([^{};]*?)\)\s*\{" % name, src)
        assert d, f"{name} not defined in mcmc.hip"
        assert len(d.group(1).split(",")) == nargs, name
        assert len(_lib._SIGS[name]) == nargs and name in _lib.exported_names()
        assert hasattr(_lib.load(), name)
        assert f"`{name}`" in doc, f"{name} missing from INTEGRATION.md"
    assert "mcmc.hip" in [s for s, _ in _build.SOURCES]
    # no environment, no allocation, no state in the new file
    for word in ("getenv", "hipMalloc", "hipFree", "static "):
        assert word not in src, word
    assert "mcmc_inject_noise_kernel" in src and "mcmc_relocation_kernel" in src


def test_hip_entry_points_refuse_cpu_tensors(gs):
    means, ls, q, l, z = noise_case(8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.mcmc.inject_noise_hip(means, ls, q, l, 1.0, 0, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        gs.mcmc.relocation_hip(torch.rand(4), torch.rand(4, 3), torch.ones(4, dtype=torch.int32))
