"""Checkpoints and the Gaussian-splat PLY on the CPU (gs.checkpoint): bit-for-bit round trips of model, optimizer,
densification and trainer state; a changed row count; save / load in the middle of a run against the uninterrupted run
(torch Adam on the CPU is deterministic, so equality is exact by construction); the refusals; the atomic write; the PLY
writer against bytes packed by hand and the reader against files no writer of ours produces."""
import dataclasses
import os
import struct
import types

import numpy as np
import pytest
import torch

N = 40


def _model(gs, n=N, sh_degree=2, num_cameras=3, seed=3, **cfg_kw):
    """tests/test_selective_adam_host.py:_tiny_model with every optional parameter group switched on"""
    g = torch.Generator().manual_seed(seed)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=sh_degree, background_color="auto", use_bilateral_grid=True,
                                    grid_shape=(4, 3, 2), **cfg_kw)
    cfg.camera_optimizer.mode = "SO3xR3"
    cfg.camera_velocity_optimizer.enabled = True
    K = (sh_degree + 1) ** 2
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), 0.1 * torch.randn(n, 3, generator=g),
                                    torch.randn(n, 4, generator=g), torch.randn(n, generator=g),
                                    torch.rand(n, 3, generator=g), 0.1 * torch.randn(n, K - 1, 3, generator=g),
                                    num_cameras=num_cameras)


def _grads(model, g):
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g)


def _step(gs, model, opts, g, selective):
    _grads(model, g)
    mask = (torch.rand(model.num_points, generator=g) < 0.6) if selective else None
    gs.training.optimizers_step(opts.values(), mask)
    model.step += 1


def _assert_same_training_state(m0, o0, m1, o1):
    assert set(o0) == set(o1)
    p0, p1 = dict(m0.named_parameters()), dict(m1.named_parameters())
    assert set(p0) == set(p1)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    for name in o0:
        assert type(o0[name]) is type(o1[name]), name
        g0, g1 = o0[name].param_groups[0], o1[name].param_groups[0]
        assert g0["lr"] == g1["lr"] and tuple(g0["betas"]) == tuple(g1["betas"]) and g0["eps"] == g1["eps"], name
        s0, s1 = o0[name].state[g0["params"][0]], o1[name].state[g1["params"][0]]
        assert type(s0["step"]) is type(s1["step"]) and float(s0["step"]) == float(s1["step"]), name
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(s0[key], s1[key]), (name, key)


@pytest.mark.parametrize("kind", ["adam", "selective_adam"])
def test_round_trip_is_bit_for_bit(gs, tmp_path, kind):
    C = gs.checkpoint
    from gsdeblur_amd import densify as D
    g = torch.Generator().manual_seed(11)
    model = _model(gs)
    opts = gs.training.make_optimizers(model, lr_scale=0.5, fused=False, optimizer=kind)
    assert set(opts) == set(model.gauss_params()) | {"camera_opt", "camera_velocity_opt", "background", "bilateral_grid"}
    for _ in range(3):
        _step(gs, model, opts, g, kind == "selective_adam")
    model.radii, model.xy_grad = torch.ones(2, N, dtype=torch.int32), torch.ones(N, 2)      # transient: not saved
    state = D.DensifyState(N, "cpu", absgrad=True)
    state.xys_grad_norm, state.vis_counts = torch.rand(N, generator=g), torch.arange(N, dtype=torch.float32)
    state.max_2Dsize, state.size = torch.rand(N, generator=g), (64, 48)
    shuffle = torch.Generator().manual_seed(5)
    order = torch.randperm(7, generator=shuffle).tolist()[:4]                               # a consumed generator
    history = [{"step": 2, "loss": 0.25, "psnr": float("inf")}]
    dcfg = D.DensifyConfig(warmup_length=4, refine_every=6)
    trainer = C.trainer_state(3, 7, shuffle, order, 2, history, 1.5, 0.5, 0.2, dcfg)
    path = tmp_path / "a.pt"
    C.save_checkpoint(path, model, opts, trainer=trainer, densify_state=state, extra={"note": "x", "k": [1, 2.5, None]})

    # the file itself: plain data, CPU tensors, readable without unpickling arbitrary objects
    raw = torch.load(path, weights_only=True)
    assert raw["format"] == "gsdeblur-checkpoint" and raw["version"] == 1
    assert isinstance(raw["model"]["config"]["grid_shape"], list)
    assert raw["model"]["config"]["camera_optimizer"] == {"mode": "SO3xR3"}
    assert isinstance(raw["optimizers"]["groups"]["means"]["step"], int)
    assert set(raw["model"]) == {"config", "num_cameras", "step", "params", "background_param", "pose_adjustment",
                                 "velocity_adjustment", "bilateral_grids"}

    ck = C.load_checkpoint(path, "cpu")
    _assert_same_training_state(model, opts, ck.model, ck.optimizers)
    assert ck.optimizers["means"].state[ck.model.means]["step"].item() == 3
    assert ck.model.step == 3 and ck.model.num_cameras == 3 and ck.model.num_points == N
    assert ck.model.config == model.config and ck.model.config.grid_shape == (4, 3, 2)
    assert ck.model.radii is None and ck.model.xy_grad is None
    assert ck.model.frame_hints is not model.frame_hints
    for k in ("xys_grad_norm", "vis_counts", "max_2Dsize"):
        assert torch.equal(getattr(ck.densify_state, k), getattr(state, k)), k
    assert ck.densify_state.size == (64, 48) and ck.densify_state.absgrad is True
    t = ck.trainer
    assert (t["iteration"], t["seed"], t["order"], t["ev_pos"]) == (3, 7, order, 2)
    assert t["history"] == history and t["wall_clock_time_seconds"] == 1.5 and t["lr_scale"] == 0.5
    assert t["ssim_lambda"] == 0.2 and t["strategy"] == "splatfacto"
    assert D.DensifyConfig(**t["strategy_config"]) == dcfg
    assert t["rng_cuda"] is None and t["rng_cpu"].dtype == torch.uint8
    assert torch.equal(t["generator_state"], shuffle.get_state())
    g2 = torch.Generator()
    g2.set_state(t["generator_state"])
    assert torch.randperm(7, generator=g2).tolist() == torch.randperm(7, generator=shuffle).tolist()
    assert ck.extra == {"note": "x", "k": [1, 2.5, None]}


def test_default_generator_state_is_saved_and_restored(gs):
    C = gs.checkpoint
    torch.manual_seed(123)
    torch.rand(5)
    tr = C.trainer_state(0, 0, None, [], 0, [], 0.0, 1.0, 0.2)
    want = torch.rand(4)
    torch.rand(100)
    C.restore_default_generators(tr, "cpu")
    assert torch.equal(torch.rand(4), want)
    assert tr["strategy"] is None and tr["strategy_config"] is None and tr["generator_state"] is None
    from gsdeblur_amd import mcmc as M
    tr = C.trainer_state(0, 0, None, [], 0, [], 0.0, 1.0, 0.2, M.MCMCConfig(cap_max=99))
    assert tr["strategy"] == "mcmc" and M.MCMCConfig(**tr["strategy_config"]).cap_max == 99


def test_changed_row_count_comes_back_with_its_moments(gs, tmp_path):
    """densify._swap_parameter on all six groups (as test_selective_step_after_a_densification_on_the_cpu does): the
    loaded model has the new N, the moments carried over, and steps"""
    C = gs.checkpoint
    from gsdeblur_amd import densify as D
    g = torch.Generator().manual_seed(2)
    model = _model(gs)
    opts = gs.training.make_optimizers(model, fused=False)
    _step(gs, model, opts, g, False)
    keep = torch.arange(N) % 5 != 0
    with torch.no_grad():
        for name, p in list(model.gauss_params().items()):
            D._swap_parameter(model, opts, name, torch.cat([p.detach()[keep], p.detach()[:3]]), keep, 3)
    N1 = int(keep.sum()) + 3
    assert model.num_points == N1 != N
    C.save_checkpoint(tmp_path / "n.pt", model, opts)
    ck = C.load_checkpoint(tmp_path / "n.pt", "cpu")
    assert ck.model.num_points == N1 and ck.trainer is None and ck.densify_state is None and ck.extra is None
    _assert_same_training_state(model, opts, ck.model, ck.optimizers)
    assert ck.optimizers["features_rest"].state[ck.model.features_rest]["exp_avg"].shape == (N1, 8, 3)
    assert not ck.optimizers["means"].state[ck.model.means]["exp_avg"][-3:].any()      # appended rows: zero moments
    ga, gb = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    _step(gs, model, opts, ga, False)
    _step(gs, ck.model, ck.optimizers, gb, False)
    _assert_same_training_state(model, opts, ck.model, ck.optimizers)


@pytest.mark.parametrize("kind", ["adam", "selective_adam"])
def test_save_load_in_the_middle_equals_the_uninterrupted_run(gs, tmp_path, kind):
    C = gs.checkpoint
    sel = kind == "selective_adam"
    a = _model(gs)
    oa = gs.training.make_optimizers(a, fused=False, optimizer=kind)
    ga = torch.Generator().manual_seed(4)
    for _ in range(6):
        _step(gs, a, oa, ga, sel)
    b = _model(gs)
    ob = gs.training.make_optimizers(b, fused=False, optimizer=kind)
    gb = torch.Generator().manual_seed(4)
    for _ in range(3):
        _step(gs, b, ob, gb, sel)
    C.save_checkpoint(tmp_path / "mid.pt", b, ob)
    ck = C.load_checkpoint(tmp_path / "mid.pt", "cpu")
    assert ck.model is not b
    for _ in range(3):
        _step(gs, ck.model, ck.optimizers, gb, sel)
    _assert_same_training_state(a, oa, ck.model, ck.optimizers)
    assert ck.model.step == 6


def test_optimizers_that_never_stepped_and_no_optimizers(gs, tmp_path):
    C = gs.checkpoint
    model = _model(gs)
    opts = gs.training.make_optimizers(model, fused=False)
    C.save_checkpoint(tmp_path / "fresh.pt", model, opts)
    ck = C.load_checkpoint(tmp_path / "fresh.pt", "cpu")
    assert all(not o.state for o in ck.optimizers.values())
    C.save_checkpoint(tmp_path / "bare.pt", model)
    ck = C.load_checkpoint(tmp_path / "bare.pt", "cpu")
    assert ck.optimizers is None and ck.trainer is None
    assert torch.equal(ck.model.bilateral_grids, model.bilateral_grids)
    with pytest.raises(TypeError, match="extra.bad"):
        C.save_checkpoint(tmp_path / "bad.pt", model, extra={"bad": object()})
    assert not (tmp_path / "bad.pt").exists()


def _rewrite(src, dst, edit):
    obj = torch.load(src, weights_only=True)
    edit(obj)
    torch.save(obj, dst)
    return dst


def test_refusals(gs, tmp_path, monkeypatch):
    C = gs.checkpoint
    g = torch.Generator().manual_seed(1)
    model = _model(gs)
    opts = gs.training.make_optimizers(model, fused=False)
    _step(gs, model, opts, g, False)
    good = tmp_path / "good.pt"
    C.save_checkpoint(good, model, opts)

    def cut_moment(o):
        o["optimizers"]["groups"]["scales"]["exp_avg_sq"] = o["optimizers"]["groups"]["scales"]["exp_avg_sq"][:-1]

    with pytest.raises(ValueError, match="unknown key 'colour_space'"):
        C.load_checkpoint(_rewrite(good, tmp_path / "k.pt", lambda o: o["model"]["config"].update(colour_space="x")), "cpu")
    with pytest.raises(ValueError, match="unknown key 'schedule'"):
        C.load_checkpoint(_rewrite(good, tmp_path / "k2.pt",
                                   lambda o: o["model"]["config"]["camera_optimizer"].update(schedule=1)), "cpu")
    with pytest.raises(ValueError, match="exp_avg_sq"):
        C.load_checkpoint(_rewrite(good, tmp_path / "m.pt", cut_moment), "cpu")
    # a missing config key takes the default: files written before a field existed still load
    old = C.load_checkpoint(_rewrite(good, tmp_path / "o.pt", lambda o: o["model"]["config"].pop("opacity_reg")), "cpu")
    assert old.model.config == model.config
    # format and version are checked before anything is built
    built = []
    monkeypatch.setattr(C, "_build_model", lambda *a, **k: built.append(1))
    monkeypatch.setattr(C, "_restore_into", lambda *a, **k: built.append(1))
    with pytest.raises(ValueError, match="format"):
        C.load_checkpoint(_rewrite(good, tmp_path / "f.pt", lambda o: o.update(format="something-else")), "cpu")
    with pytest.raises(ValueError, match="version"):
        C.load_checkpoint(_rewrite(good, tmp_path / "v.pt", lambda o: o.update(version=2)), "cpu")
    with pytest.raises(ValueError, match="format"):
        torch.save([1, 2], tmp_path / "l.pt")
        C.load_checkpoint(tmp_path / "l.pt", "cpu")
    assert not built


def test_a_file_that_needs_full_unpickling_is_not_loaded(gs, tmp_path):
    import pickle
    torch.save({"format": "gsdeblur-checkpoint", "version": 1, "model": types.SimpleNamespace()}, tmp_path / "p.pt")
    with pytest.raises(pickle.UnpicklingError):
        gs.checkpoint.load_checkpoint(tmp_path / "p.pt", "cpu")


def test_restore_into_an_existing_model(gs, tmp_path):
    C = gs.checkpoint
    g = torch.Generator().manual_seed(1)
    model = _model(gs, n=25)
    opts = gs.training.make_optimizers(model, fused=False)
    _step(gs, model, opts, g, False)
    C.save_checkpoint(tmp_path / "c.pt", model, opts)
    other = _model(gs, n=N, seed=8)
    hints = other.frame_hints
    ck = C.load_checkpoint(tmp_path / "c.pt", into=other)
    assert ck.model is other and other.num_points == 25 and other.frame_hints is hints
    _assert_same_training_state(model, opts, other, ck.optimizers)
    with pytest.raises(ValueError, match="sh_degree"):
        C.load_checkpoint(tmp_path / "c.pt", into=_model(gs, sh_degree=1))
    with pytest.raises(ValueError, match="cameras"):
        C.load_checkpoint(tmp_path / "c.pt", into=_model(gs, num_cameras=2))


def test_a_failed_save_leaves_the_previous_file_and_no_temporary(gs, tmp_path, monkeypatch):
    C = gs.checkpoint
    model = _model(gs)
    path = tmp_path / "ck" / "model.pt"
    C.save_checkpoint(path, model, extra={"n": 1})
    real = C._serialize

    def half_way(obj, f):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(C, "_serialize", half_way)
    first = model.means.detach().clone()
    with torch.no_grad():
        model.means.add_(1.0)
    with pytest.raises(OSError, match="disk full"):
        C.save_checkpoint(path, model, extra={"n": 2})
    assert os.listdir(path.parent) == ["model.pt"]
    ck = C.load_checkpoint(path, "cpu")
    assert ck.extra == {"n": 1} and torch.equal(ck.model.means, first)
    monkeypatch.setattr(C, "_serialize", real)
    C.save_checkpoint(path, model, extra={"n": 3})
    assert os.listdir(path.parent) == ["model.pt"] and C.load_checkpoint(path, "cpu").extra == {"n": 3}


# --------------------------------------------------------------------------- #
# train_scene: checkpoint_path / checkpoint_every / resume with a CPU stand-in for the render
# --------------------------------------------------------------------------- #
H, W = 16, 16


def _cpu_scene(gs):
    cams = [gs.Camera(torch.eye(4)[:3], 10.0, 10.0, 8.0, 8.0, W, H, metadata={"cam_idx": i}) for i in range(5)]
    images = [torch.full((H, W, 3), 0.15 + 0.15 * i) for i in range(5)]
    return types.SimpleNamespace(cameras=cams, train_indices=[1, 2, 3, 4], eval_indices=[0]), images


def _cpu_trainable(gs, n=30):
    g = torch.Generator().manual_seed(3)
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, background_color="auto")
    cfg.camera_optimizer.mode = "SO3xR3"
    model = gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.zeros(n, 3), torch.randn(n, 4, generator=g),
                                     torch.zeros(n), torch.rand(n, 3, generator=g), torch.zeros(n, 3, 3), num_cameras=5)

    def fake_outputs(camera, **kw):
        i = camera.metadata["cam_idx"]
        w = torch.zeros(model.num_points, 1)
        w[i * 5:i * 5 + 12] = 1.0
        col = (model.features_dc * w).mean(0) + 0.01 * (model.means * w).sum() + 0.01 * (model.scales * w).sum() \
            + 0.01 * (model.quats * w).sum() + 0.01 * (model.opacities * w).sum() + 0.01 * (model.features_rest * w[..., None]).sum() \
            + torch.sigmoid(model.background_param) * 0.1 + model.pose_adjustment[i].sum()
        model.radii = (w.reshape(1, -1) > 0).to(torch.int32)
        return {"rgb": col[None, None, :].expand(H, W, 3), "depth": None}

    model.get_outputs = fake_outputs
    return model


def _flat_state(model, opts):
    out = {k: p.detach().clone() for k, p in model.named_parameters()}
    for name, o in opts.items():
        st = o.state[o.param_groups[0]["params"][0]]
        out[name + ".m"], out[name + ".v"], out[name + ".t"] = st["exp_avg"], st["exp_avg_sq"], torch.tensor(float(st["step"]))
    return out


@pytest.mark.parametrize("kind", ["adam", "selective_adam"])
def test_train_scene_resume_equals_the_uninterrupted_run_on_the_cpu(gs, tmp_path, monkeypatch, kind):
    C, T = gs.checkpoint, gs.training
    scene, images = _cpu_scene(gs)
    kept = {}
    real_make = T.make_optimizers

    def spy(model, *a, **k):
        kept[id(model)] = real_make(model, *a, **k)
        return kept[id(model)]

    monkeypatch.setattr(T, "make_optimizers", spy)
    kw = dict(ssim_lambda=0.0, log_every=2, seed=6, optimizer=kind, optimize_eval_cameras=True, eval_camera_every=3,
              lr_scale=2.0)
    a = _cpu_trainable(gs)
    res_a = T.train_scene(a, scene, images, 10, **kw)
    b = _cpu_trainable(gs)
    res_b1 = T.train_scene(b, scene, images, 5, checkpoint_path=tmp_path / "b.pt", **kw)
    assert res_b1["history"] == res_a["history"][:2]
    tr = torch.load(tmp_path / "b.pt", weights_only=True)["trainer"]
    assert tr["iteration"] == 5 and tr["seed"] == 6 and tr["ev_pos"] == 1 and len(tr["order"]) == 3 and tr["lr_scale"] == 2.0
    c = _cpu_trainable(gs)
    res_c = T.train_scene(c, scene, images, 10, resume=tmp_path / "b.pt", ssim_lambda=0.0, log_every=2,
                          optimize_eval_cameras=True, eval_camera_every=3)
    assert res_c["history"] == res_a["history"] and len(res_a["history"]) == 5
    assert res_c["results"] == res_a["results"]
    assert res_c["wall_clock_time_seconds"] >= res_b1["wall_clock_time_seconds"]
    sa, sc = _flat_state(a, kept[id(a)]), _flat_state(c, kept[id(c)])
    assert set(sa) == set(sc)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert a.step == c.step == 10
    assert kept[id(c)]["means"].param_groups[0]["lr"] == 2.0 * 1.6e-4
    assert type(kept[id(c)]["means"]).__name__ == ("SelectiveAdam" if kind == "selective_adam" else "Adam")
    with pytest.raises(ValueError, match="strategy"):
        T.train_scene(_cpu_trainable(gs), scene, images, 10, resume=tmp_path / "b.pt", ssim_lambda=0.0,
                      densify=gs.mcmc.MCMCConfig())


def test_train_scene_checkpoint_every_saves_on_schedule_and_defaults_save_nothing(gs, tmp_path, monkeypatch):
    C, T = gs.checkpoint, gs.training
    scene, images = _cpu_scene(gs)
    saved = []
    real = C.save_checkpoint
    monkeypatch.setattr(C, "save_checkpoint", lambda path, *a, **k: (saved.append(k["trainer"]["iteration"]), real(path, *a, **k)))
    T.train_scene(_cpu_trainable(gs), scene, images, 10, ssim_lambda=0.0, checkpoint_path=tmp_path / "e.pt",
                  checkpoint_every=4)
    assert saved == [4, 8, 10]
    del saved[:]
    T.train_scene(_cpu_trainable(gs), scene, images, 3, ssim_lambda=0.0)
    assert saved == [] and sorted(os.listdir(tmp_path)) == ["e.pt"]
    with pytest.raises(ValueError, match="checkpoint_path"):
        T.train_scene(_cpu_trainable(gs), scene, images, 3, ssim_lambda=0.0, checkpoint_every=2)


# --------------------------------------------------------------------------- #
# Gaussian-splat PLY
# --------------------------------------------------------------------------- #
def _header(n, rest):
    """the expected header, written out here independently of the writer"""
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += ["f_rest_%d" % i for i in range(rest)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    text = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    text += "".join("property float %s\n" % nm for nm in names) + "end_header\n"
    return text.encode("ascii")


def _ply_model(gs, sh_degree, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    K = (sh_degree + 1) ** 2
    cfg = gs.SplatfactoDeblurConfig(sh_degree=sh_degree)
    return gs.SplatfactoDeblurModel(cfg, torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g),
                                    torch.randn(n, 4, generator=g), torch.randn(n, generator=g),
                                    torch.randn(n, 3, generator=g), torch.randn(n, K - 1, 3, generator=g))


def test_export_ply_known_answer_at_degree_1(gs, tmp_path):
    means = [[1.0, 2.0, 3.0], [-4.0, 5.5, -6.25], [0.125, -0.5, 7.0]]
    scales = [[-1.0, -2.0, -3.0], [-1.5, -2.5, -3.5], [0.25, 0.5, 0.75]]
    quats = [[1.0, 0.0, 0.0, 0.0], [0.5, -0.5, 0.5, -0.5], [2.0, 3.0, 4.0, 5.0]]
    opac = [-2.0, 0.0, 3.5]
    dc = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]]
    rest = [[[100.0 * n + 10.0 * k + c for c in range(3)] for k in range(3)] for n in range(3)]     # [n][k][c]
    model = gs.SplatfactoDeblurModel(gs.SplatfactoDeblurConfig(sh_degree=1), torch.tensor(means), torch.tensor(scales),
                                     torch.tensor(quats), torch.tensor(opac), torch.tensor(dc), torch.tensor(rest))
    want = _header(3, 9)
    for n in range(3):
        f_rest = [rest[n][k][c] for c in range(3) for k in range(3)]                 # channel-major: index c * 3 + k
        row = means[n] + [0.0, 0.0, 0.0] + dc[n] + f_rest + [opac[n]] + scales[n] + quats[n]
        assert len(row) == 26
        want += struct.pack("<26f", *row)
    assert f_rest[1] == 210.0 and f_rest[3] == 201.0
    written = gs.checkpoint.export_ply(tmp_path / "s.ply", model)
    assert written == 3
    assert (tmp_path / "s.ply").read_bytes() == want
    assert os.listdir(tmp_path) == ["s.ply"]


@pytest.mark.parametrize("sh_degree,rest", [(0, 0), (3, 45)])
def test_export_ply_file_length(gs, tmp_path, sh_degree, rest):
    n = 7
    model = _ply_model(gs, sh_degree, n)
    assert gs.checkpoint.export_ply(tmp_path / "s.ply", model) == n
    raw = (tmp_path / "s.ply").read_bytes()
    header = _header(n, rest)
    assert raw.startswith(header) and len(raw) == len(header) + n * 4 * (17 + rest)
    assert (b"f_rest" in raw[:len(header)]) == (rest > 0)


@pytest.mark.parametrize("sh_degree", [0, 1, 2, 3])
def test_ply_round_trip_is_bit_for_bit(gs, tmp_path, sh_degree):
    model = _ply_model(gs, sh_degree, 9, seed=sh_degree)
    gs.checkpoint.export_ply(tmp_path / "s.ply", model)
    d = gs.checkpoint.load_ply(tmp_path / "s.ply")
    assert d["sh_degree"] == sh_degree
    for k, p in model.gauss_params().items():
        assert d[k].dtype == torch.float32 and torch.equal(d[k], p.detach()), k
    back = gs.SplatfactoDeblurModel.from_ply(tmp_path / "s.ply")
    assert back.config.sh_degree == sh_degree and back.background_param is None and back.pose_adjustment is None
    for k, p in model.gauss_params().items():
        assert torch.equal(dict(back.gauss_params())[k], p), k
    cfg = gs.SplatfactoDeblurConfig(sh_degree=sh_degree, rasterize_mode="classic")
    assert gs.SplatfactoDeblurModel.from_ply(tmp_path / "s.ply", cfg, num_cameras=4).num_cameras == 4
    with pytest.raises(ValueError, match="SH degree"):
        gs.SplatfactoDeblurModel.from_ply(tmp_path / "s.ply", gs.SplatfactoDeblurConfig(sh_degree=sh_degree + 1))


def _foreign_ply(model, path, fmt="binary_little_endian 1.0", drop=(), extra_rest=0, cut=0, comment=True):
    """the model's Gaussians in a file as another program might write it: columns in a shuffled order, an extra uchar
    and an extra double column, opacity stored as double, new-style type names, a comment line, CRLF-free header"""
    n = model.num_points
    rest = model.features_rest.detach().permute(0, 2, 1).reshape(n, -1).numpy()
    cols = {"x": model.means[:, 0], "y": model.means[:, 1], "z": model.means[:, 2]}
    for i in range(3):
        cols[f"f_dc_{i}"] = model.features_dc[:, i]
        cols[f"scale_{i}"] = model.scales[:, i]
    for i in range(4):
        cols[f"rot_{i}"] = model.quats[:, i]
    cols = {k: v.detach().numpy() for k, v in cols.items()}
    for i in range(rest.shape[1]):
        cols[f"f_rest_{i}"] = rest[:, i]
    for i in range(extra_rest):
        cols[f"f_rest_{rest.shape[1] + i}"] = np.zeros(n, np.float32)
    cols["opacity"] = model.opacities.detach().numpy()[:, 0].astype(np.float64)
    cols["label"] = (np.arange(n) % 250).astype(np.uint8)
    cols["confidence"] = np.linspace(0.0, 1.0, n)
    names = sorted(cols, key=lambda s: (hash_order(s), s))
    names = [nm for nm in names if nm not in drop]
    tname = {"float32": "float32", "float64": "double", "uint8": "uchar"}
    dtype = np.dtype([(nm, cols[nm].dtype.newbyteorder("<")) for nm in names])
    table = np.zeros(n, dtype)
    for nm in names:
        table[nm] = cols[nm]
    head = ["ply", f"format {fmt}"] + (["comment written by another program"] if comment else [])
    head += [f"element vertex {n}"] + [f"property {tname[cols[nm].dtype.name]} {nm}" for nm in names]
    head += ["element face 0", "property list uchar int vertex_indices", "end_header"]
    body = table.tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii") + body[:len(body) - cut])
    return names


def hash_order(s):
    """a fixed shuffle of the column names (no dependence on PYTHONHASHSEED)"""
    return sum((i + 3) * ord(c) for i, c in enumerate(s)) % 7


def test_load_ply_finds_columns_by_name_and_skips_what_it_does_not_know(gs, tmp_path):
    model = _ply_model(gs, 2, 11, seed=5)
    names = _foreign_ply(model, tmp_path / "f.ply")
    assert names[:3] != ["x", "y", "z"] and "label" in names and "nx" not in names
    d = gs.checkpoint.load_ply(tmp_path / "f.ply")
    assert d["sh_degree"] == 2
    for k, p in model.gauss_params().items():
        assert torch.equal(d[k], p.detach()), k


def test_load_ply_refusals(gs, tmp_path):
    C = gs.checkpoint
    model = _ply_model(gs, 1, 6)
    p = tmp_path / "f.ply"
    _foreign_ply(model, p, drop=("opacity",))
    with pytest.raises(ValueError, match="opacity"):
        C.load_ply(p)
    _foreign_ply(model, p, drop=("rot_3", "x"))
    with pytest.raises(ValueError, match="rot_3"):
        C.load_ply(p)
    for fmt in ("ascii 1.0", "binary_big_endian 1.0"):
        _foreign_ply(model, p, fmt=fmt)
        with pytest.raises(ValueError, match="binary_little_endian"):
            C.load_ply(p)
    _foreign_ply(model, p, cut=1)
    with pytest.raises(ValueError, match="truncated"):
        C.load_ply(p)
    _foreign_ply(model, p, extra_rest=1)                     # 10 f_rest columns: no SH degree has that many
    with pytest.raises(ValueError, match="f_rest"):
        C.load_ply(p)
    _foreign_ply(model, p, drop=("f_rest_4",))               # 8 columns with a hole
    with pytest.raises(ValueError, match="f_rest"):
        C.load_ply(p)
    p.write_bytes(b"not a ply at all")
    with pytest.raises(ValueError, match="PLY"):
        C.load_ply(p)
    _foreign_ply(model, p)                                   # the same file without a defect loads
    assert C.load_ply(p)["means"].shape == (6, 3)


def test_export_ply_drops_and_counts_non_finite_rows(gs, tmp_path):
    model = _ply_model(gs, 1, 8)
    with torch.no_grad():
        model.scales[2, 1] = float("inf")
        model.features_rest[5, 2, 0] = float("nan")
    written = gs.checkpoint.export_ply(tmp_path / "s.ply", model)
    assert written == 6
    d = gs.checkpoint.load_ply(tmp_path / "s.ply")
    keep = [0, 1, 3, 4, 6, 7]
    for k, p in model.gauss_params().items():
        assert torch.equal(d[k], p.detach()[keep]), k


def test_the_checkpoint_of_a_config_lists_every_field(gs):
    """a field added to SplatfactoDeblurConfig travels without a change to checkpoint.py"""
    cfg = gs.SplatfactoDeblurConfig(sh_degree=2, grid_shape=(8, 4, 2))
    d = gs.checkpoint.config_to_dict(cfg)
    assert set(d) == {f.name for f in dataclasses.fields(cfg)}
    assert gs.checkpoint.config_from_dict(d) == cfg
    assert gs.checkpoint.config_from_dict({}) == gs.SplatfactoDeblurConfig()
