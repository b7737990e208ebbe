"""Selective Adam on the CPU: the torch SelectiveAdam against a float64 reference and torch.optim.Adam, the config
defaults, the C-ABI entries of gs_adam_step_rows / gs_visible_rows, train_step's row masks on the CPU route, and a
world-2 gloo run whose ranks see different Gaussians and must stay bit-identical."""
import os
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
NEW_EXPORTS = ("gs_adam_step_rows", "gs_adam_step_rows_workspace_bytes", "gs_visible_rows")


def _ref64_step(p, g, m, v, mask, lr, b1, b2, eps, step):
    p, g, m, v = (t.double().clone() for t in (p, g, m, v))
    m2 = m + (g - m) * (1 - b1)
    v2 = v * b2 + (1 - b2) * g * g
    p2 = p - lr / (1 - b1 ** step) * m2 / (v2.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    sel = mask.reshape(-1, *([1] * (p.dim() - 1)))
    return torch.where(sel, p2, p), torch.where(sel, m2, m), torch.where(sel, v2, v)


def test_selective_adam_all_true_mask_equals_torch_adam(gs):
    SelectiveAdam = gs.training.SelectiveAdam
    g = torch.Generator().manual_seed(0)
    shapes = [(257, 3), (257, 15, 3), (257, 1)]
    a = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    b = [torch.nn.Parameter(x.detach().clone()) for x in a]
    oa = torch.optim.Adam(a, lr=3e-3, eps=1e-15)
    ob = SelectiveAdam(b, lr=3e-3, eps=1e-15)
    full = torch.ones(257, dtype=torch.bool)
    for _ in range(5):
        for x, y in zip(a, b):
            x.grad = torch.randn(x.shape, generator=g)
            y.grad = x.grad.clone()
        oa.step()
        ob.step(full)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[x][k], ob.state[y][k]), k


def test_selective_adam_against_float64_with_changing_masks(gs):
    SelectiveAdam = gs.training.SelectiveAdam
    g = torch.Generator().manual_seed(1)
    N = 300
    p = torch.nn.Parameter(torch.randn(N, 4, generator=g))
    cam = torch.nn.Parameter(torch.randn(5, 6, generator=g))        # another leading dimension: steps densely
    opt = SelectiveAdam([p, cam], lr=1e-2, betas=(0.9, 0.999), eps=1e-15)
    m = torch.zeros(N, 4, dtype=torch.float64)
    v = torch.zeros(N, 4, dtype=torch.float64)
    ref = p.detach().double().clone()
    for step in range(1, 7):
        mask = torch.rand(N, generator=g) < (0.1 if step % 2 else 0.6)
        p.grad = torch.randn(N, 4, generator=g)
        cam.grad = torch.randn(5, 6, generator=g)
        before = (p.detach().clone(), opt.state[p]["exp_avg"].clone() if opt.state[p] else torch.zeros(N, 4),
                  opt.state[p]["exp_avg_sq"].clone() if opt.state[p] else torch.zeros(N, 4))
        cam0 = cam.detach().clone()
        opt.step(mask)
        st = opt.state[p]
        # masked-off rows: bit-identical parameter and moments
        assert torch.equal(p.detach()[~mask], before[0][~mask])
        assert torch.equal(st["exp_avg"][~mask], before[1][~mask])
        assert torch.equal(st["exp_avg_sq"][~mask], before[2][~mask])
        # selected rows: Adam with the GLOBAL step's bias correction (gsplat's rule)
        ref, m, v = _ref64_step(ref, p.grad, m, v, mask, 1e-2, 0.9, 0.999, 1e-15, step)
        assert torch.allclose(p.detach().double(), ref, rtol=1e-5, atol=1e-6)
        assert torch.allclose(st["exp_avg"].double(), m, rtol=1e-5, atol=1e-8)
        assert torch.allclose(st["exp_avg_sq"].double(), v, rtol=1e-5, atol=1e-10)
        assert float(st["step"]) == step
        assert not torch.equal(cam.detach(), cam0)                     # dense parameter moved in full
        ref = p.detach().double().clone()                              # follow the float32 trajectory
        m, v = st["exp_avg"].double().clone(), st["exp_avg_sq"].double().clone()


def _tiny_model(gs, n=40, **cfg_kw):
    g = torch.Generator().manual_seed(3)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, **cfg_kw)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.zeros(n, 3),
                                    torch.randn(n, 4, generator=g), torch.zeros(n), torch.rand(n, 3, generator=g),
                                    torch.zeros(n, 3, 3), num_cameras=2)


def test_config_defaults_and_make_optimizers_unchanged(gs):
    cfg = gs.SplatfactoDeblurConfig()
    assert cfg.optimizer == "adam" and cfg.selective_mask == "visible"
    model = _tiny_model(gs, background_color="auto")
    opts = gs.training.make_optimizers(model)
    assert all(type(o) is torch.optim.Adam for o in opts.values())
    assert set(opts) == set(model.gauss_params()) | {"background"}
    sel = gs.training.make_optimizers(model, optimizer="selective_adam")
    for k in model.gauss_params():
        assert type(sel[k]) is gs.training.SelectiveAdam
    assert type(sel["background"]) is torch.optim.Adam
    with pytest.raises(ValueError):
        gs.training.make_optimizers(model, optimizer="sgd")
    # with plain Adam no mask is built
    assert gs.training.selection_mask(model, opts.values()) is None


def _strip(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_new_exports_in_header_definitions_and_ctypes_table(gs):
    from gsdeblur_amd import _lib
    hdr = _strip((ROOT / "include" / "gsdeblur.h").read_text())
    src = _strip((ROOT / "3dgs-deblur_amd" / "csrc" / "train.hip").read_text())
    want = {"gs_adam_step_rows": 16, "gs_adam_step_rows_workspace_bytes": 1, "gs_visible_rows": 5}
    for name, nargs in want.items():
        m = re.search(r"\b%s\s*\(([^;{}]*?)\)\s*;" % name, hdr)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == nargs, name
        d = re.search(r"GS_EXPORT\s+[\w\s\*]+?\b%s\s*\(([^{};]*?)\)\s*\{" % name, src)
        assert d, f"{name} not defined in train.hip"
        assert len(d.group(1).split(",")) == nargs, name
        table = _lib._SIGS_LL if name.endswith("_bytes") else _lib._SIGS
        assert len(table[name]) == nargs, name
        assert name in _lib.exported_names()
    # appended after gs_adam_step, which keeps its prototype
    assert hdr.index("gs_adam_step(") < hdr.index("gs_adam_step_rows(")
    assert "int gs_adam_step(int count, float* const* params" in hdr


def test_selection_mask_on_the_cpu_route(gs):
    """visible = radii > 0 in any plane (one camera [P,N], a batch [B,P,N], a list of per-camera planes); touched = any
    non-zero gradient row"""
    model = _tiny_model(gs, optimizer="selective_adam")
    opts = gs.training.make_optimizers(model)
    N = model.num_points
    r = torch.zeros(3, N, dtype=torch.int32)
    r[0, 5] = 2
    r[2, 9] = 1
    r[1, 11] = -1
    model.radii = r
    want = torch.zeros(N, dtype=torch.bool)
    want[[5, 9]] = True
    assert torch.equal(gs.training.selection_mask(model, opts.values()), want)
    model.radii = torch.stack([r, torch.zeros_like(r)])
    assert torch.equal(gs.training.selection_mask(model, opts.values()), want)
    model.radii = [r[:1], r[1:]]
    assert torch.equal(gs.training.selection_mask(model, opts.values()), want)
    model.radii = torch.zeros(3, N + 1, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        gs.training.selection_mask(model, opts.values())
    model.config.selective_mask = "touched"
    for p in model.gauss_params().values():
        p.grad = torch.zeros_like(p)
    model.means.grad[3, 1] = 1.0
    model.features_rest.grad[17, 2, 0] = -2.0
    want = torch.zeros(N, dtype=torch.bool)
    want[[3, 17]] = True
    assert torch.equal(gs.training.selection_mask(model, opts.values()), want)


def test_selective_step_after_a_densification_on_the_cpu(gs):
    """densify._swap_parameter changes N and carries the moments; the next step's mask is built at the new N"""
    from gsdeblur_amd import densify as D
    model = _tiny_model(gs, optimizer="selective_adam", selective_mask="visible")
    opts = gs.training.make_optimizers(model)
    N0 = model.num_points
    for p in model.gauss_params().values():
        p.grad = torch.ones_like(p)
    model.radii = torch.ones(2, N0, dtype=torch.int32)
    gs.training.optimizers_step(opts.values(), gs.training.selection_mask(model, opts.values()))
    keep = torch.arange(N0) % 5 != 0
    with torch.no_grad():
        for name, p in list(model.gauss_params().items()):
            D._swap_parameter(model, opts, name, torch.cat([p.detach()[keep], p.detach()[:3]]), keep, 3)
    N1 = model.num_points
    assert N1 == int(keep.sum()) + 3
    before = {k: p.detach().clone() for k, p in model.gauss_params().items()}
    for p in model.gauss_params().values():
        p.grad = torch.ones_like(p)
    r = torch.zeros(2, N1, dtype=torch.int32)
    r[1, ::2] = 3
    model.radii = r
    mask = gs.training.selection_mask(model, opts.values())
    assert mask.shape == (N1,)
    gs.training.optimizers_step(opts.values(), mask)
    for k, p in model.gauss_params().items():
        assert torch.equal(p.detach()[~mask], before[k][~mask]), k
        assert not torch.equal(p.detach()[mask], before[k][mask]), k
        assert opts[k].state[p]["exp_avg"].shape == p.shape


def _dp_selective_worker(rank, world, port, q):
    """train_step's DP branch with a CPU stand-in render whose radii differ per rank: the "visible" mask is MAX-reduced
    over the ranks, so parameters and moments stay bit-identical"""
    sys.path.insert(0, str(ROOT))
    import gsdeblur_amd as gs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, H, W = 64, 8, 8
    g = torch.Generator().manual_seed(3)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, optimizer="selective_adam", selective_mask="visible")
    model = gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.zeros(n, 3), torch.randn(n, 4, generator=g),
                                     torch.zeros(n), torch.rand(n, 3, generator=g), torch.zeros(n, 3, 3), num_cameras=2)
    opts = gs.training.make_optimizers(model)

    def fake_outputs(camera):
        i = camera.metadata["cam_idx"]
        w = torch.zeros(n, 1)
        w[i * 20:i * 20 + 24] = 1.0                         # every view touches its own Gaussians ...
        radii = torch.zeros(2, n, dtype=torch.int32)
        radii[1, i * 20:i * 20 + 30] = 4                    # ... and sees a few more
        model.radii = radii
        col = (model.features_dc * w).sum(0) + model.means.mul(w).sum() * 0.01 + model.scales.mul(w).sum() * 0.01
        rgb = (0.1 * col)[None, None, :].expand(H, W, 3)
        return {"rgb": rgb}

    model.get_outputs = fake_outputs
    c2w = torch.eye(4)[:3]
    untouched = []
    for step in range(4):
        i = (step + rank) % 2                               # the ranks render DIFFERENT views
        cam = gs.Camera(c2w, 10.0, 10.0, 4.0, 4.0, W, H, metadata={"cam_idx": i})
        target = torch.full((H, W, 3), 0.2 + 0.5 * i)
        before = model.means.detach().clone()
        gs.training.train_step(model, opts, cam, target, ssim_lambda=0.0, allreduce="sparse")
        untouched.append(torch.equal(model.means.detach()[60:], before[60:]))   # seen by no view of any rank
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()] +
                     [opts[k].state[p][s].reshape(-1) for k, p in model.gauss_params().items()
                      for s in ("exp_avg", "exp_avg_sq")])
    other = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(other, flat)
    same = all(torch.equal(o, flat) for o in other)
    q.put((rank, same, all(untouched)))
    dist.destroy_process_group()


def test_selective_adam_world2_gloo_visible_mask_keeps_replicas_identical():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_selective_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True, True), (1, True, True)]
