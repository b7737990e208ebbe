"""Checkpoints and the Gaussian-splat PLY on the GPU: a loaded model renders the saved model's image bit for bit, so does
a model built from the exported PLY; a run that is saved at step 12, loaded into a fresh model and resumed ends where the
uninterrupted run ends (three densification variants); HipAdam state loads into torch.optim.Adam and back; and
tools/render_model.py writes the reference's file names and training.evaluate's numbers.

The bar of the resume tests does not come from the checkpoint code: the uninterrupted run is made TWICE and the two are
compared first (test_uninterrupted_run_repeats_bit_for_bit)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ITERS, SAVE_AT = 24, 12
VARIANTS = ("plain", "densify", "mcmc")


@pytest.fixture(scope="module")
def world(gs, dev, tmp_path_factory):
    import synthetic_dataset as SD          # tools/synthetic_dataset.py (conftest puts tools/ on sys.path)
    tmp = tmp_path_factory.mktemp("ckpt")
    root = str(tmp / "ds")
    SD.generate(root, dev, width=64, height=48, n_frames=8, n_gaussians=3000, speed=1.0, dense_samples=8,
                seed_points=1500)
    scene = gs.load_transforms(root)
    images = gs.data.load_scene_images(scene, dev)
    xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
    return {"SD": SD, "root": root, "tmp": tmp, "scene": scene, "images": images, "xyz": xyz, "rgb": rgb, "runs": {}}


def _variant(gs, name):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=3, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, background_color="black")
    dcfg = None
    if name == "densify":
        # num_train_data=1: the post-reset guard (step % 180 > num_train_data + refine_every) lets step 12 refine, so N
        # changes BEFORE the save; step 6 resets the opacities
        dcfg = gs.densify.DensifyConfig(warmup_length=4, refine_every=6, num_train_data=1, densify_grad_thresh=2e-4)
    elif name == "mcmc":
        cfg.opacity_reg = cfg.scale_reg = 0.01
        dcfg = gs.mcmc.MCMCConfig(cap_max=2000, refine_every=6, refine_start_iter=4)
    return cfg, dcfg


def _state(model, opts):
    out = {k: p.detach().clone() for k, p in model.named_parameters()}
    for name, o in opts.items():
        st = o.state[o.param_groups[0]["params"][0]]
        out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        out[name + ".step"] = torch.tensor(float(st["step"]))
    return out


def _train(gs, world, name, iterations, fresh_hints_after=None, **kw):
    """train_scene on a fresh model -> (model, optimizers, result); fresh_hints_after=k replaces model.frame_hints by a
    fresh ops.FrameHints() once step k is done — what a model loaded at step k starts with"""
    from gsdeblur_amd import ops
    T = gs.training
    cfg, dcfg = _variant(gs, name)
    model = world["SD"].init_from_seed_points(cfg, world["xyz"], world["rgb"], world["images"][0].device,
                                              num_cameras=len(world["scene"].cameras))
    real_make, real_step = T.make_optimizers, T.train_step
    box, calls = {}, [0]

    def make(m, *a, **k):
        box["opts"] = real_make(m, *a, **k)
        return box["opts"]

    def step(m, *a, **k):
        h = real_step(m, *a, **k)
        calls[0] += 1
        if fresh_hints_after is not None and calls[0] == fresh_hints_after:
            m.frame_hints = ops.FrameHints()
        return h

    T.make_optimizers, T.train_step = make, step
    try:
        res = T.train_scene(model, world["scene"], world["images"], iterations, densify=dcfg, log_every=4, seed=1, **kw)
    finally:
        T.make_optimizers, T.train_step = real_make, real_step
    return model, box["opts"], res


def _runs(gs, world, name):
    """per variant, once: run A twice (uninterrupted, fresh hints after step 12), run B (12 steps, save; a fresh model
    resumes to 24)"""
    if name not in world["runs"]:
        r = {}
        for tag in ("a1", "a2"):
            m, o, res = _train(gs, world, name, ITERS, fresh_hints_after=SAVE_AT)
            r[tag] = {"state": _state(m, o), "res": res, "n": m.num_points}
        path = world["tmp"] / f"{name}.pt"
        m, o, res = _train(gs, world, name, SAVE_AT, checkpoint_path=path)
        r["b1"] = {"model": m, "opts": o, "res": res, "path": path, "n": m.num_points}
        m, o, res = _train(gs, world, name, ITERS, resume=path)
        r["b2"] = {"state": _state(m, o), "res": res, "n": m.num_points}
        world["runs"][name] = r
    return world["runs"][name]


def _rel_diff(x, y):
    """per tensor: max |x - y| relative to the tensor's max magnitude (inf when the shapes differ)"""
    out = {}
    for k in x:
        if x[k].shape != y[k].shape:
            out[k] = float("inf")
        elif x[k].numel():
            out[k] = float((x[k] - y[k]).abs().max() / x[k].abs().max().clamp(min=1e-30))
        else:
            out[k] = 0.0
    return out


@pytest.mark.parametrize("name", VARIANTS)
def test_uninterrupted_run_repeats_bit_for_bit(gs, dev, world, name):
    """Run A against run A: 24 steps, the same process, the same inputs.  The backward sums per-Gaussian tuples with plain
    stores in a fixed order (reduce_tuples_*) and the optimizer is elementwise, so the run is expected to
    repeat exactly; this is the measurement the resume test's bar rests on.  Observed on the MI355X: every parameter, both
    moments of every optimizer and every step count torch.equal in all three variants (max relative difference 0;
    N at the end 1500 / 2517 / 2000) — DESIGN §5.8."""
    r = _runs(gs, world, name)
    d = _rel_diff(r["a1"]["state"], r["a2"]["state"])
    print(f"A-vs-A [{name}] N = {r['a1']['n']}: max relative difference {max(d.values()):.3e} "
          f"({max(d, key=d.get)}); non-zero in {sorted(k for k, v in d.items() if v)}")
    assert set(r["a1"]["state"]) == set(r["a2"]["state"])
    for k, t in r["a1"]["state"].items():
        assert torch.equal(t, r["a2"]["state"][k]), (k, d[k])
    assert r["a1"]["res"]["history"] == r["a2"]["res"]["history"]


@pytest.mark.parametrize("name", VARIANTS)
def test_resume_equals_the_uninterrupted_run(gs, dev, world, name):
    """Run B (12 steps, save, load into a fresh model and fresh optimizers, resume to 24) against run A.  Run A repeats
    bit for bit (the test above), so the bar is torch.equal on every parameter, both moments and the step
    counts.  Observed on the MI355X: N at the save 1500 / 1193 / 2000, A-versus-B difference 0 in every tensor."""
    r = _runs(gs, world, name)
    n_saved = int(torch.load(r["b1"]["path"], weights_only=True)["model"]["params"]["means"].shape[0])
    print(f"resume [{name}]: N 1500 -> {n_saved} at the save -> {r['b2']['n']} at the end")
    if name != "plain":
        assert n_saved != 1500                        # the row count changed before the save
    assert r["b1"]["n"] == n_saved
    d = _rel_diff(r["a1"]["state"], r["b2"]["state"])
    print(f"A-vs-B [{name}]: max relative difference {max(d.values()):.3e} ({max(d, key=d.get)})")
    assert set(r["a1"]["state"]) == set(r["b2"]["state"])
    for k, t in r["a1"]["state"].items():
        assert torch.equal(t, r["b2"]["state"][k]), (k, d[k])
    a, b = r["a1"]["res"], r["b2"]["res"]
    assert [h["step"] for h in b["history"]] == [4, 8, 12, 16, 20, 24]
    assert b["history"][:3] == r["b1"]["res"]["history"]
    assert b["history"] == a["history"] and b["results"] == a["results"]
    assert b["wall_clock_time_seconds"] > r["b1"]["res"]["wall_clock_time_seconds"]


def _render(model, camera):
    from gsdeblur_amd import ops
    model.eval()
    model.frame_hints = ops.FrameHints()
    out = model.get_outputs_for_camera(camera)
    return out["rgb"], out["depth"]


@pytest.mark.parametrize("name", VARIANTS)
def test_loaded_model_renders_the_same_image(gs, dev, world, name):
    r = _runs(gs, world, name)
    src = r["b1"]["model"]
    ck = gs.checkpoint.load_checkpoint(r["b1"]["path"], dev)
    assert ck.model is not src and ck.model.means.is_cuda and ck.model.num_points == src.num_points
    assert ck.model.step == SAVE_AT and ck.trainer["iteration"] == SAVE_AT
    assert type(ck.optimizers["means"]).__name__ == "HipAdam" and ck.optimizers["means"].state[ck.model.means]["step"] == SAVE_AT
    assert (ck.densify_state is not None) == (name == "densify")
    cam = world["scene"].cameras[world["scene"].eval_indices[0]]
    rgb0, depth0 = _render(src, cam)
    rgb1, depth1 = _render(ck.model, cam)
    assert rgb0.abs().sum() > 0 and torch.isfinite(depth0).all()
    assert torch.equal(rgb0, rgb1) and torch.equal(depth0, depth1)


@pytest.mark.parametrize("name", ["plain", "mcmc"])
def test_model_from_exported_ply_renders_the_same_image(gs, dev, world, name):
    """zero velocity, no pose adjustment: those do not travel in a PLY"""
    r = _runs(gs, world, name)
    src = r["b1"]["model"]
    path = world["tmp"] / f"{name}.ply"
    assert gs.checkpoint.export_ply(path, src) == src.num_points
    assert path.stat().st_size == len(gs.checkpoint.ply_header(src.num_points, 45)) + 248 * src.num_points
    back = gs.SplatfactoDeblurModel.from_ply(path, src.config, dev, num_cameras=src.num_cameras)
    for k, p in src.gauss_params().items():
        assert torch.equal(dict(back.gauss_params())[k], p), k
    cam = world["scene"].cameras[world["scene"].eval_indices[0]]
    assert not any(cam.metadata["camera_linear_velocity"]) and not any(cam.metadata["camera_angular_velocity"])
    rgb0, depth0 = _render(src, cam)
    rgb1, depth1 = _render(back, cam)
    assert torch.equal(rgb0, rgb1) and torch.equal(depth0, depth1)


def test_hip_adam_state_loads_into_torch_adam_and_back(gs, dev, world):
    C = gs.checkpoint
    r = _runs(gs, world, "densify")
    src, opts = r["b1"]["model"], r["b1"]["opts"]
    cpu = C.load_checkpoint(r["b1"]["path"], "cpu")
    assert not cpu.model.means.is_cuda and not cpu.densify_state.vis_counts.is_cuda
    for k, p in src.gauss_params().items():
        o = cpu.optimizers[k]
        assert type(o) is torch.optim.Adam
        st, st_gpu = o.state[dict(cpu.model.gauss_params())[k]], opts[k].state[p]
        assert isinstance(st_gpu["step"], int) and st_gpu["step"] == SAVE_AT
        assert isinstance(st["step"], torch.Tensor) and not st["step"].is_cuda and int(st["step"]) == SAVE_AT
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[key], st_gpu[key].cpu()), (k, key)
        assert o.param_groups[0]["lr"] == opts[k].param_groups[0]["lr"]
    # the other way round: written from torch.optim.Adam state, loaded into HipAdam, one step on the GPU
    back_path = world["tmp"] / "from_cpu.pt"
    C.save_checkpoint(back_path, cpu.model, cpu.optimizers)
    gpu = C.load_checkpoint(back_path, dev)
    assert type(gpu.optimizers["means"]).__name__ == "HipAdam"
    st = gpu.optimizers["scales"].state[gpu.model.scales]
    assert st["step"] == SAVE_AT and torch.equal(st["exp_avg_sq"], opts["scales"].state[src.scales]["exp_avg_sq"])
    before = gpu.model.means.detach().clone()
    i = world["scene"].train_indices[0]
    h = gs.training.train_step(gpu.model, gpu.optimizers, world["scene"].cameras[i], world["images"][i])
    torch.cuda.synchronize()
    assert st["step"] == SAVE_AT + 1 and gpu.model.step == SAVE_AT + 1
    assert torch.isfinite(gpu.model.means).all() and not torch.equal(gpu.model.means.detach(), before)
    assert h["loss"] == h["loss"]


def test_render_model_tool_writes_the_reference_names_and_evaluates_numbers(gs, dev, world):
    r = _runs(gs, world, "plain")
    out = world["tmp"] / "renders"
    proc = subprocess.run([sys.executable, str(ROOT / "tools" / "render_model.py"), "--checkpoint", str(r["b1"]["path"]),
                           "--data", world["root"], "--set", "eval", "--out", str(out)],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    scene = world["scene"]
    stems = [Path(scene.image_paths[i]).stem for i in scene.eval_indices]
    assert sorted(p.name for p in out.glob("*_pred.png")) == sorted(f"{s}_pred.png" for s in stems)
    assert sorted(p.name for p in out.glob("*_gt.png")) == sorted(f"{s}_gt.png" for s in stems)
    assert sorted(p.name for p in (out / "pred" / "depth" / "raw").iterdir()) == sorted(f"{s}.npy" for s in stems)
    import numpy as np
    depth = np.load(out / "pred" / "depth" / "raw" / f"{stems[0]}.npy")
    assert depth.shape == (48, 64, 1) and np.isfinite(depth).all()
    assert tuple(gs.data.load_image(str(out / f"{stems[0]}_pred.png")).shape) == (48, 64, 3)
    got = json.loads((out / "metrics.json").read_text())["results"]
    model = gs.checkpoint.load_checkpoint(r["b1"]["path"], dev).model
    want = gs.training.evaluate(model, scene.cameras, world["images"], scene.eval_indices)
    print(f"render_model.py: psnr {got['psnr']!r} ssim {got['ssim']!r}; training.evaluate: {want}")
    assert abs(got["psnr"] - want["psnr"]) <= 1e-6 and abs(got["ssim"] - want["ssim"]) <= 1e-6
