"""SH degrees other than 3 on the host: the progressive schedule, the model / optimizers / densification row surgery /
sparse exchange with the zero-width features_rest of degree 0 and the 72-wide one of degree 4 (CPU tensors), and the
float64 oracle itself at (active degree, allocated K) — the reference side of tests/test_gpu_sh_degrees.py."""
import math
import multiprocessing as mp
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import sh_degree_cases as C

ROOT = Path(__file__).resolve().parent.parent


def _model(gs, degree, n=12, interval=0, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    K = (degree + 1) ** 2
    cfg = gs.SplatfactoDeblurConfig(sh_degree=degree, sh_degree_interval=interval, **kw)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.full((n, 3), math.log(0.01)),
                                    torch.ones(n, 4), torch.zeros(n), torch.randn(n, 3, generator=g),
                                    torch.randn(n, K - 1, 3, generator=g), 4)


# --------------------------------------------------------------------------- the progressive schedule
@pytest.mark.parametrize("degree,interval", [(3, 2), (4, 1), (3, 1000), (0, 5)])
def test_active_sh_degree_follows_the_schedule_in_training_only(gs, degree, interval):
    model = _model(gs, degree, interval=interval)
    for step in (0, 1, interval - 1, interval, 2 * interval, 3 * interval + 1, 4 * interval, 10 * interval, 10 ** 6):
        model.step = step
        model.train()
        assert model.active_sh_degree() == min(step // interval, degree), step
        model.eval()
        assert model.active_sh_degree() == degree, step                  # evaluation renders every band


@pytest.mark.parametrize("degree", [0, 1, 4])
def test_interval_0_means_all_bands_at_once(gs, degree):
    model = _model(gs, degree, interval=0)
    for step in (0, 1, 999, 10 ** 6):
        model.step = step
        model.train()
        assert model.active_sh_degree() == degree
        model.eval()
        assert model.active_sh_degree() == degree
    assert gs.SplatfactoDeblurConfig().sh_degree_interval == 0


def test_train_step_hands_the_active_degree_to_the_render(gs, monkeypatch):
    """the CPU route of train_step with a stand-in render: the degree it is asked for follows model.step, and the
    gradient of features_rest keeps the allocated shape"""
    model = _model(gs, 3, interval=2)
    seen = []

    def stand_in(camera, **kw):
        seen.append(model.active_sh_degree())
        nb = (seen[-1] + 1) ** 2
        rgb = (model.features_dc.sum() + model.features_rest[:, :nb - 1].sum() + model.means.sum()
               + model.scales.sum() + model.quats.sum() + model.opacities.sum()) * torch.ones(16, 16, 3) * 1e-3
        return {"rgb": rgb, "depth": None}

    monkeypatch.setattr(model, "get_outputs", stand_in)
    opts = gs.training.make_optimizers(model)
    rest0 = model.features_rest.detach().clone()
    for it in range(8):
        gs.training.train_step(model, opts, None, torch.zeros(16, 16, 3), 0.0)
        nb = (seen[-1] + 1) ** 2
        gr = model.features_rest.grad
        assert gr.shape == (12, 15, 3) and not gr[:, nb - 1:].any()
        assert torch.equal(model.features_rest.detach()[:, nb - 1:], rest0[:, nb - 1:])
    assert seen == [0, 0, 1, 1, 2, 2, 3, 3]


# --------------------------------------------------------------------------- degree 0 / degree 4 on the CPU model path
@pytest.mark.parametrize("degree", [0, 4])
@pytest.mark.parametrize("optimizer", ["adam", "selective_adam"])
def test_cpu_model_optimizers_and_row_surgery(gs, degree, optimizer):
    """features_rest [N,0,3] / [N,24,3]: parameter and gradient shapes, optimizer construction, a (selective) step, and
    densify._swap_parameter's cull + duplicate with the Adam moments carried along"""
    from gsdeblur_amd import densify as D
    n, K = 12, (degree + 1) ** 2
    model = _model(gs, degree, n, optimizer=optimizer)
    assert model.features_rest.shape == (n, K - 1, 3) and model.features_rest.numel() == n * (K - 1) * 3
    opts = gs.training.make_optimizers(model, fused=False)
    assert set(model.gauss_params()) <= set(opts)
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(n, generator=g) < 0.5
    mask[0], mask[1] = True, False
    before = {k: p.detach().clone() for k, p in model.gauss_params().items()}
    for p in model.gauss_params().values():
        p.grad = torch.randn(p.shape, generator=g)
    assert model.features_rest.grad.shape == (n, K - 1, 3)
    gs.training.optimizers_step(opts.values(), row_mask=mask if optimizer == "selective_adam" else None)
    for k, p in model.gauss_params().items():
        st = opts[k].state[p]
        assert st["exp_avg"].shape == p.shape and bool(torch.isfinite(p).all()), k
        if optimizer == "selective_adam":
            assert torch.equal(p.detach()[~mask], before[k][~mask]), k
        if p.numel():
            assert not torch.equal(p.detach()[mask], before[k][mask]), k
    keep = torch.ones(n, dtype=torch.bool)
    keep[::5] = False
    dup = torch.arange(0, n, 4)
    with torch.no_grad():
        for name, p in list(model.gauss_params().items()):
            m0 = opts[name].state[p]["exp_avg"].clone()
            D._swap_parameter(model, opts, name, torch.cat([p.detach()[keep], p.detach()[dup]]), keep, dup.numel())
            q = model.gauss_params()[name]
            st = opts[name].state[q]
            assert q.shape[0] == int(keep.sum()) + dup.numel() and q.shape[1:] == p.shape[1:], name
            assert st["exp_avg"].shape == q.shape and torch.equal(st["exp_avg"][:int(keep.sum())], m0[keep]), name
            assert not st["exp_avg"][int(keep.sum()):].any(), name             # new rows start without momentum
    assert model.features_rest.shape == (model.num_points, K - 1, 3)
    # and the next step runs on the new rows
    for p in model.gauss_params().values():
        p.grad = torch.randn(p.shape, generator=g)
    mask2 = torch.rand(model.num_points, generator=g) < 0.5
    gs.training.optimizers_step(opts.values(), row_mask=mask2 if optimizer == "selective_adam" else None)
    assert all(bool(torch.isfinite(p).all()) for p in model.gauss_params().values())


def test_cpu_row_ops_with_a_zero_width_tensor(gs):
    """dp._RowOps (the torch form the HIP row kernels are tested against) with features_rest [N,0,3]: no payload
    column, pack -> scatter_add reproduces the rows"""
    from gsdeblur_amd.dp import _RowOps
    N = 500
    g = torch.Generator().manual_seed(2)
    touched = torch.rand(N, generator=g) < 0.1
    shapes = [(N, 3), (N, 4), (N,), (N, 3), (N, 0, 3)]
    grads = [torch.randn(s, generator=g) * touched.view(-1, *([1] * (len(s) - 1))) for s in shapes]
    ops_ = _RowOps(grads)
    assert ops_.widths == [3, 4, 1, 3, 0] and ops_.wtot == 11
    assert torch.equal(ops_.row_mask(), touched)
    idx = touched.nonzero().reshape(-1)
    pay = ops_.pack(idx, idx.numel() + 3)
    assert pay.shape == (idx.numel() + 3, 12)
    acc = _RowOps([torch.zeros(s) for s in shapes])
    acc.scatter_add(pay, idx.numel(), 1.0)
    for a, b in zip(acc.grads, grads):
        assert a.shape == b.shape and torch.equal(a, b)
    pm = ops_.pack_masked(idx.numel() + 5)
    acc2 = _RowOps([torch.zeros(s) for s in shapes])
    acc2.scatter_add_payload(pm, idx.numel() + 5, 2.0)
    for a, b in zip(acc2.grads, grads):
        assert torch.equal(a, 2.0 * b)


def _sparse_worker(rank, world, port, q, rest_width):
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    import gsdeblur_amd as gs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    N = 6000
    shapes = [(N, 3), (N, 3), (N, 4), (N, 1), (N, 3), (N, rest_width, 3)]
    ok = True
    for step, density in enumerate((0.01, 0.02, 0.5, 0.01)):
        gens = [torch.Generator().manual_seed(50 + 7 * step + r) for r in range(world)]
        all_grads = []
        for r in range(world):
            touched = torch.rand(N, generator=gens[r]) < density
            all_grads.append([torch.randn(s, generator=gens[r]) * touched.view(-1, *([1] * (len(s) - 1))) for s in shapes])
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        for p, g in zip(params, all_grads[rank]):
            p.grad = g.clone()
        gs.dp.allreduce_gradients(params, mode="sparse")
        for i, p in enumerate(params):
            want = sum(all_grads[r][i] for r in range(world))
            ok &= p.grad.shape == shapes[i] and bool(torch.allclose(p.grad, want, atol=1e-6))
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.parametrize("rest_width", [0, 24])
def test_sparse_exchange_over_gloo_with_degree_0_and_4_shapes(rest_width):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 47300 + (os.getpid() % 2000) + rest_width
    procs = [ctx.Process(target=_sparse_worker, args=(r, 2, port, q, rest_width)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]


# --------------------------------------------------------------------------- the reference side
@pytest.mark.parametrize("deg,K", C.CASES)
def test_oracle_sh_with_more_coefficients_than_the_degree_uses(oracle, deg, K):
    """spherical_harmonics(deg, dirs, coeffs [N,K,3]) uses coeffs[:, :nb] only: same colours as on the cut tensor, and the
    unused bands get exact-zero gradients"""
    O = oracle
    g = torch.Generator().manual_seed(deg * 100 + K)
    n, nb = 200, C.nb_of(deg)
    dirs = torch.randn(n, 3, generator=g, dtype=torch.float64)
    co = torch.randn(n, K, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    cut = co.detach()[:, :nb].clone().requires_grad_(True)
    a = O.spherical_harmonics(deg, dirs, co)
    b = O.spherical_harmonics(deg, dirs, cut)
    assert torch.equal(a, b)
    w = torch.randn(n, 3, generator=g, dtype=torch.float64)
    (a * w).sum().backward()
    (b * w).sum().backward()
    assert torch.equal(co.grad[:, :nb], cut.grad) and not co.grad[:, nb:].any()
    assert bool((co.grad[:, :nb].abs().amax(dim=(0, 2)) > 0).all())


@pytest.mark.parametrize("deg,K", [(1, 16), (2, 25)])
def test_oracle_frame_ignores_the_unused_bands(oracle, deg, K):
    """a whole oracle frame at (deg, K) against the frame of the cut tensor: the same image, sh gradients of the used
    bands equal, of the unused bands exactly zero (what the GPU tests then demand of the kernels)"""
    O = oracle
    nb = C.nb_of(deg)
    sc = C.scene(O, deg, K, n=300)
    f = C.oracle_frame(O, sc, deg)
    wt = C.loss_weights(f["frag"])
    (f["ref"] * wt.double()).sum().backward()
    sc2 = dict(sc)
    sc2["sh"] = sc["sh"][:, :nb].clone()
    f2 = C.oracle_frame(O, sc2, deg)
    (f2["ref"] * wt.double()).sum().backward()
    assert torch.equal(f["ref"], f2["ref"]) and torch.equal(f["frag"], f2["frag"])
    gsh = f["q"]["sh"].grad
    assert torch.equal(gsh[:, :nb], f2["q"]["sh"].grad) and not gsh[:, nb:].any()
    for k in ("means", "log_scales", "quats", "opacity_logits", "viewmat", "lin_vel", "ang_vel"):
        assert torch.equal(f["q"][k].grad, f2["q"][k].grad), k


@pytest.mark.parametrize("deg,K", [(0, 16), (4, 25)])
def test_recorded_oracle_shares(oracle, deg, K):
    """the shares recorded in sh_degree_cases.FRAGILE_OBSERVED are the oracle's own, re-derived here for two cases; the
    colour clamp is active and the colour-clamp-fragile rows stay under their cap"""
    f = C.oracle_frame(oracle, C.scene(oracle, deg, K), deg)
    share = float(f["frag"].float().mean())
    print(f"[{C.tag(deg, K)}] fragile {share:.5f}, per sample {float(f['frag_s'].float().mean()):.5f}, on the clamp "
          f"{f['clamped']:.4f}, clamp-fragile rows {int(f['clamp_rows'].sum())}")
    assert abs(share - C.FRAGILE_OBSERVED[(deg, K)]) < 5e-4
    assert f["clamped"] >= C.CLAMPED_MIN and int(f["clamp_rows"].sum()) <= C.CLAMP_ROWS_MAX * C.N
    assert float(f["frag_s"].float().mean()) < 0.01


def test_degree_4_finite_difference_of_the_oracle_sh_gradient(oracle):
    """autograd through the float64 oracle at degree 4 against central differences of sh coefficients from every band
    (as test_oracle.test_finite_difference_gradients, which stops at degree 3), on a scene with the cases' DC x2 /
    rest x6 scaling so that clamped colours are among them: a clamped channel must have zero on both sides"""
    O = oracle
    Wd, Hd, n = 32, 32, 40
    sc = O.synthetic_scene(n, Wd, Hd, seed=9, scale_mult=10.0, sh_degree=4)
    sh = sc["sh"].double().clone()
    sh[:, 0] *= 2.0
    sh[:, 1:] *= 6.0
    cfg = O.RenderConfig(Hd, Wd, sc["fx"], sc["fy"], sc["cx"], sc["cy"], sh_degree=4, blur_samples=2, rs_bands=2,
                         exposure_time=0.02, rolling_shutter_time=0.02, gamma=2.2, min_rgb_level=5.0, upstream_grads=0)
    names = ["log_scales", "quats", "opacity_logits"]
    ps = {k: sc[k].double().clone().requires_grad_(True) for k in names}
    ps["sh"] = sh.clone().requires_grad_(True)
    wt = torch.rand(Hd, Wd, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))

    def loss(p):
        out, _ = O.render(cfg, sc["means"].double(), p["log_scales"].exp(), p["quats"], torch.sigmoid(p["opacity_logits"]),
                          p["sh"], sc["viewmat"].double(), sc["lin_vel"].double(), sc["ang_vel"].double())
        return (out * wt).sum()

    loss(ps).backward()
    g = ps["sh"].grad
    assert bool((g.abs().amax(dim=(0, 2)) > 0).all())                   # every one of the 25 bands gets a gradient
    rng = np.random.default_rng(0)
    eps = 1e-6
    worst, zeros = 0.0, 0
    for band in range(25):
        rows = np.flatnonzero(g[:, band].abs().amax(dim=1).numpy() > 0)
        picks = [(int(rng.choice(rows)), int(rng.integers(3)))] + [(int(rng.integers(n)), int(rng.integers(3)))]
        for row, ch in picks:
            def at(delta):
                q = {kk: vv.detach().clone() for kk, vv in ps.items()}
                q["sh"][row, band, ch] += delta
                return loss(q).item()
            fd = (at(eps) - at(-eps)) / (2 * eps)
            an = g[row, band, ch].item()
            if an == 0.0:
                zeros += 1
                assert abs(fd) < 1e-9, (row, band, ch, fd)               # clamped or unseen: flat on both sides
                continue
            worst = max(worst, abs(fd - an) / (abs(an) + abs(fd) + 1e-5))
    print(f"degree-4 sh finite differences: worst relative error {worst:.2e}, {zeros} exact-zero elements among the picks")
    assert worst < 5e-4, worst                                          # test_finite_difference_gradients' bar
