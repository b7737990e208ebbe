"""3DGS-MCMC on the MI355X: gs_mcmc_relocation and gs_mcmc_inject_noise against the float64 reference
(tests/mcmc_reference.py), the Philox stream's statistics and determinism, train_scene with an MCMCConfig through both
optimizers, and the end-to-end comparison with a run without densification."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mcmc_reference as R
from test_mcmc_host import (assert_delta_close, assert_relocation_close, mh, noise_case, relocation_grid,  # noqa: F401
                            P)

pytestmark = pytest.mark.gpu


# ---- relocation ---------------------------------------------------------------------------------------------------
def test_relocation_kernel_on_the_grid_and_on_random_rows(gs, dev):
    o, s, n = relocation_grid()
    new_o, new_s = gs.mcmc.relocation_hip(o.to(dev), s.to(dev), n.to(dev))
    assert_relocation_close(new_o.cpu(), new_s.cpu(), o, s, n)
    one = n == 1
    assert ((new_o.cpu()[one] - o[one]).abs() <= 1e-6 * o[one]).all()
    assert ((new_s.cpu()[one] - s[one]).abs() <= 1e-6 * s[one]).all()
    a = gs.mcmc.relocation_hip(o[n == 51].to(dev), s[n == 51].to(dev), n[n == 51].to(dev))
    b = gs.mcmc.relocation_hip(o[n == 51].to(dev), s[n == 51].to(dev), torch.full_like(n[n == 51], 400).to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                  # n > 51 is n = 51
    M = 100_003
    g = torch.Generator().manual_seed(12)
    o = torch.exp(torch.empty(M).uniform_(math.log(0.005), math.log(0.999), generator=g))
    s = torch.exp(torch.empty(M, 3).uniform_(math.log(1e-4), math.log(2.0), generator=g))
    n = torch.randint(1, 60, (M,), generator=g, dtype=torch.int32)
    new_o, new_s = gs.mcmc.relocation_hip(o.to(dev), s.to(dev), n.to(dev))
    assert_relocation_close(new_o.cpu(), new_s.cpu(), o, s, n)
    e = gs.mcmc.relocation_hip(o[:0].to(dev), s[:0].to(dev), n[:0].to(dev))     # M == 0: a no-op
    assert e[0].shape == (0,) and e[1].shape == (0, 3)
    L = gs._lib.load()
    assert L.gs_mcmc_relocation(0, None, None, None, None, None, None) == 0


# ---- noise with caller-supplied normals -------------------------------------------------------------------------------
def _raw_inject(gs, N, means, ls, q, l, scaler, seed, step, noise_in, noise_out):
    """the C entry itself, with N smaller than the buffers"""
    L = gs._lib.load()
    vp = ctypes.c_void_p
    st = L.gs_mcmc_inject_noise(N, vp(means.data_ptr()), vp(ls.data_ptr()), vp(q.data_ptr()), vp(l.data_ptr()),
                                float(scaler), seed, step, vp(noise_in.data_ptr() if noise_in is not None else None),
                                vp(noise_out.data_ptr() if noise_out is not None else None),
                                vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("N", [1, 63, 64, 65, 100_003, 0])
def test_noise_kernel_with_noise_in_against_float64(gs, dev, N):
    pad = 70                                               # rows beyond N: must stay untouched
    means, ls, q, l, z = noise_case(N + pad, seed=N)
    scaler = 5e5 * 1.6e-4
    m = means.to(dev)
    used = torch.full((N + pad, 3), -7.0, device=dev)
    assert _raw_inject(gs, N, m, ls.to(dev), q.to(dev), l.to(dev), scaler, 0, 0, z.to(dev), used) == 0
    assert torch.equal(m.cpu()[N:], means[N:])
    assert torch.equal(used.cpu()[N:], torch.full((pad, 3), -7.0))
    if N == 0:
        return
    assert torch.equal(used.cpu()[:N], z[:N])
    ref = R.noise_delta(ls[:N], q[:N], l[:N], z[:N], scaler)
    # the kernel adds the displacement to the mean in fp32: recover it in float64 up to half an ulp of the mean, and
    # check the displacement itself on means of zero
    m0 = torch.zeros(N, 3, device=dev)
    assert _raw_inject(gs, N, m0, ls[:N].to(dev), q[:N].to(dev), l[:N].to(dev), scaler, 0, 0, z[:N].to(dev), None) == 0
    assert_delta_close(m0.cpu(), ref)
    assert ((m.cpu()[:N].double() - means[:N].double()) - ref).abs().max() <= \
        1.2e-7 * (means[:N].abs().max() + ref.abs().max()) + 1e-4 * ref.abs().max()


def test_noise_through_the_python_binding_equals_the_raw_call(gs, dev):
    N = 5000
    means, ls, q, l, z = (t.to(dev) for t in noise_case(N, seed=3))
    a, b = means.clone(), means.clone()
    gs.mcmc.inject_noise_hip(a, ls, q, l, 80.0, 0, 0, noise_in=z)
    assert _raw_inject(gs, N, b, ls, q, l, 80.0, 0, 0, z, None) == 0
    assert torch.equal(a, b) and not torch.equal(a, means)


# ---- noise from the Philox stream --------------------------------------------------------------------------------------
def test_philox_noise_statistics_displacement_and_determinism(gs, dev, mh):  # noqa: F811
    N = 2 ** 20
    means, ls, q, l, _ = (t.to(dev) for t in noise_case(N, seed=21))
    means.zero_()
    scaler = 80.0

    def run(seed, step):
        m, used = means.clone(), torch.empty(N, 3, device=dev)
        gs.mcmc.inject_noise_hip(m, ls, q, l, scaler, seed, step, noise_out=used)
        return m, used
    m, z = run(0, 0)
    zd = z.double()
    n = float(N)
    mean, var = zd.mean(dim=0), zd.var(dim=0, unbiased=False)
    c = torch.corrcoef(zd.T)
    print("philox normals: mean", mean.tolist(), "var", var.tolist(), "corr", [c[0, 1].item(), c[0, 2].item(),
                                                                             c[1, 2].item()], "max", z.abs().max().item())
    assert torch.isfinite(z).all()
    assert (mean.abs() < 5 / math.sqrt(n)).all()
    assert ((var - 1).abs() < 5 * math.sqrt(2 / n)).all()
    assert max(abs(c[0, 1].item()), abs(c[0, 2].item()), abs(c[1, 2].item())) < 5 / math.sqrt(n)
    assert z.abs().max().item() <= 6.8
    # the displacement is the reference applied to the normals the kernel reports
    ref = R.noise_delta(ls.cpu(), q.cpu(), l.cpu(), z.cpu(), scaler)
    assert_delta_close(m.cpu(), ref)
    # a function of (seed, step, row) alone
    m2, z2 = run(0, 0)
    assert torch.equal(m, m2) and torch.equal(z, z2)
    for seed, step in ((0, 1), (1, 0), (0, 2 ** 32), (2 ** 32, 0)):
        _, zo = run(seed, step)
        assert not torch.equal(z, zo), (seed, step)
        assert (zo == z).float().mean().item() < 1e-3
    # ... and the same words as the host build of the header: rows 0 .. 1023 of key 0, step 0
    k = 1024
    w = np.zeros((k, 4), np.uint32)
    mh.mh_row_words(k, ctypes.c_ulonglong(0), ctypes.c_ulonglong(0), P(w))
    assert [int(x) for x in w[0]] == R.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c,
                                                                               0x9b00dbd8]
    zh = np.zeros((k, 3), np.float32)
    mh.mh_normals(k, P(w), P(zh))
    assert float((z[:k].cpu() - torch.from_numpy(zh)).abs().max()) < 1e-5
    assert float((z[:k].cpu().double() - R.normals_from_words(torch.from_numpy(w.astype(np.int64)))).abs().max()) < 1e-5


def test_relocate_and_add_on_gpu_tensors_go_through_the_kernels(gs, dev, monkeypatch):
    """the strategy on GPU tensors with HipAdam: same invariants as on the CPU, and the torch forms are never called"""
    from test_mcmc_host import _model
    model = _model(gs, 3000, seed=5).to(dev)
    opts = gs.training.make_optimizers(model)
    assert type(opts["means"]).__name__ == "HipAdam"
    for p in model.gauss_params().values():
        p.grad = torch.ones_like(p)
    gs.training.optimizers_step(opts.values())

    def boom(*a, **k):
        raise AssertionError("torch form used on GPU tensors")
    monkeypatch.setattr(gs.mcmc, "relocation_torch", boom)
    monkeypatch.setattr(gs.mcmc, "inject_noise_torch", boom)
    with torch.no_grad():
        model.opacities[::3] = -9.0
    cfg = gs.mcmc.MCMCConfig(cap_max=4000, refine_start_iter=0, refine_every=1)
    before = model.means.detach().clone()
    res = gs.mcmc.step_callback(model, opts, 5, cfg)
    assert res == {"relocated": 1000, "added": 750, "before": 3000, "after": 3750}
    assert not (torch.sigmoid(model.opacities.detach()) <= cfg.min_opacity).any()
    for k, p in model.gauss_params().items():
        st = opts[k].state[p]
        assert p.shape[0] == 3750 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert float(st["exp_avg"][3000:].abs().sum()) == 0
    assert torch.isfinite(model.means).all() and torch.isfinite(model.scales).all()
    assert before.shape != model.means.shape
    for p in model.gauss_params().values():
        p.grad = torch.ones_like(p)
    gs.training.optimizers_step(opts.values())               # the optimizers step at the new N
    res = gs.mcmc.step_callback(model, opts, 6, cfg)
    assert res["after"] == 4000


# ---- training --------------------------------------------------------------------------------------------------------
def _dataset(gs, dev, tmp_path, **kw):
    import synthetic_dataset as SD          # tools/synthetic_dataset.py (conftest puts tools/ on sys.path)
    root = str(tmp_path / "ds")
    SD.generate(root, dev, **kw)
    scene = gs.load_transforms(root)
    images = gs.data.load_scene_images(scene, dev)
    xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
    return SD, scene, images, xyz, rgb


def _spy_callback(gs, monkeypatch, log):
    real = gs.mcmc.step_callback

    def spy(model, optimizers, step, cfg, group=None):
        r = real(model, optimizers, step, cfg, group)
        n = model.num_points
        for k, p in model.gauss_params().items():
            st = optimizers[k].state[p]
            assert p.shape[0] == n and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, k
        log.append(n)
        return r
    monkeypatch.setattr(gs.mcmc, "step_callback", spy)


@pytest.mark.parametrize("optimizer", ["adam", "selective_adam"])
def test_train_scene_with_mcmc_config(gs, dev, tmp_path, monkeypatch, optimizer):
    SD, scene, images, xyz, rgb = _dataset(gs, dev, tmp_path, width=128, height=96, n_frames=8, n_gaussians=2000,
                                           speed=1.0, dense_samples=8, seed_points=400)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=2, blur_samples=3, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, opacity_reg=0.01, scale_reg=0.01,
                                    optimizer=optimizer, selective_mask="visible")
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    n0 = model.num_points
    log = []
    _spy_callback(gs, monkeypatch, log)
    mc = gs.mcmc.MCMCConfig(cap_max=900, refine_start_iter=10, refine_stop_iter=70, refine_every=10)
    r = gs.training.train_scene(model, scene, images, 80, densify=mc, optimizer=optimizer)
    assert len(log) == 80 and log == sorted(log) and max(log) <= 900 and log[0] == n0
    assert model.num_points == 900                          # 400 * 1.25^4 > 900: the cap is reached and held
    assert model.xy_grad is None and model.collect_densify_stats is False
    assert all(torch.isfinite(p).all() for p in model.gauss_params().values())
    assert math.isfinite(r["results"]["psnr"])


def test_mcmc_end_to_end_fixed_budget(gs, dev, tmp_path, monkeypatch):
    """The dataset, seed cloud and 1500 iterations of test_densification_end_to_end_grows_the_model_and_pays_on_sharp_frames,
    schedule scaled the same way: "plain" (no densification) against MCMC with cap_max = 8000 and both regularisers at
    0.01.  Quality is compared with the plain run of the same test, never with a stored number.
    Observed on the MI355X, three runs of this test: plain 19.402 dB / 0.7100, MCMC 20.433 dB / 0.7745 — a gain of
    +1.031 dB and +0.0644 SSIM, the same in all three (on this scene the run repeated bit for bit); dead share 3.6 %
    (profiles/mcmc_train.jsonl).  The test asserts half of the smallest observed gain in each."""
    SD, scene, images, xyz, rgb = _dataset(gs, dev, tmp_path, width=240, height=160, n_frames=24, n_gaussians=8000,
                                           speed=1.0, dense_samples=32, seed_points=1500)
    iters, res = 1500, {}
    log = []
    _spy_callback(gs, monkeypatch, log)
    mc = gs.mcmc.MCMCConfig(cap_max=8000, refine_start_iter=200, refine_every=100, refine_stop_iter=int(0.9 * iters))
    dead = None
    for name, dcfg, reg in (("plain", None, 0.0), ("mcmc", mc, 0.01)):
        cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                        rolling_shutter_compensation=False, use_scale_regularization=True,
                                        opacity_reg=reg, scale_reg=reg)
        model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
        r = gs.training.train_scene(model, scene, images, iters, densify=dcfg)
        res[name] = (r["results"]["psnr"], r["results"]["ssim"], model.num_points)
        if dcfg is not None:
            dead = float((torch.sigmoid(model.opacities.detach()) <= mc.min_opacity).float().mean())
            assert model.xy_grad is None
    print("sharp-frame scores (psnr, ssim, gaussians):", {k: (round(v[0], 3), round(v[1], 4), v[2]) for k, v in res.items()},
          "gain", round(res["mcmc"][0] - res["plain"][0], 3), round(res["mcmc"][1] - res["plain"][1], 4),
          "dead share", round(dead, 4))
    assert res["plain"][2] == 1500 and res["mcmc"][2] == 8000
    assert len(log) == iters and max(log) <= 8000 and log == sorted(log)
    assert dead < 0.05
    assert res["mcmc"][0] > res["plain"][0] + 0.515 and res["mcmc"][1] > res["plain"][1] + 0.0322
