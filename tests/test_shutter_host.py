"""Learnable exposure / readout times on the CPU: the time tangent of the screw interpolation (gs_math.h::
subpose_tangent_dot, the per-item arithmetic of subpose_bwd_kernel) compiled with g++ against float64 autograd through
matrix_exp (tests/shutter_reference.py); ops.subpose_times against the host schedule; the model's parameters, refusals,
fallback times, optimizer group, eval-frame rule and checkpoints."""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import shutter_reference as SR

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_math" / "shutter_host.cpp"
LIB = ROOT / "tests" / "host_math" / "libshutter_host.so"
HDR = ROOT / "3dgs-deblur_amd" / "csrc" / "gs_math.h"


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def sh():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        # -ffp-contract=off: as csrc/project.hip is compiled
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", f"-I{HDR.parent}",
                               str(SRC), "-o", str(LIB)])
    return ctypes.CDLL(str(LIB))


@pytest.fixture(scope="module")
def V0(oracle):
    # the mid-exposure pose of tests/test_host_math.py's scene
    return oracle.subpose_viewmats(torch.eye(4, dtype=torch.float64), torch.tensor([0.1, 0.05, -0.2], dtype=torch.float64),
                                   torch.tensor([0.05, -0.08, 0.03], dtype=torch.float64), [1.0])[0].float()


def _host(sh, V, lin, ang, times, go):
    n = len(times)
    Vn, ln, an = (np.ascontiguousarray(t.numpy(), np.float32) for t in (V, lin, ang))
    tn = np.ascontiguousarray(np.asarray(times, np.float32))
    gn = np.ascontiguousarray(go.numpy().reshape(n, 16), np.float32)
    vV, vl, va, vt, vc = (np.zeros(k, np.float32) for k in (16, 3, 3, n, n))
    sh.sh_subpose_bwd_times(n, P(Vn), P(ln), P(an), P(tn), P(gn), P(vV), P(vl), P(va), P(vt))
    sh.sh_subpose_time_closed(n, P(Vn), P(ln), P(an), P(tn), P(gn), P(vc))
    return vV, vl, va, vt, vc


def _cotangent(n, seed=3):
    go = torch.randn(n, 4, 4, generator=torch.Generator().manual_seed(seed))
    go[:, 3, :] = 0
    return go


CASES = {
    "P1_t0": ([0.0], (0.1, 0.05, -0.2), (0.05, -0.08, 0.03)),                  # gradient -xi^ V, not zero
    "P4_mixed_signs": ([-0.01, 0.0, 0.02, -0.3], (0.1, 0.05, -0.2), (0.05, -0.08, 0.03)),
    "zero_ang": ([-0.01, 0.0, 0.02, 0.5], (0.1, 0.05, -0.2), (0.0, 0.0, 0.0)),  # th2 == 0: series branch
    "closed_form_branch": ([0.5, -0.5, 0.45], (0.8, -0.5, 1.1), (0.9, -1.2, 0.5)),   # |ang t| = 0.79 >= 0.5
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_time_tangent_vs_float64_matrix_exp(sh, V0, case):
    """rel < 1e-5, the bar of test_se3_closed_form_vs_matrix_exp — for the time gradient AND for the 18 camera tangents
    computed by the same function; and the dual chain against the closed form -<v_out, xi^ V_p>"""
    times, lin, ang = CASES[case]
    lin, ang = torch.tensor(lin), torch.tensor(ang)
    if case == "closed_form_branch":
        assert float(ang.norm()) * min(abs(t) for t in times) >= 0.5
    go = _cotangent(len(times))
    vV, vl, va, vt, vc = _host(sh, V0, lin, ang, times, go)
    gV, gl, ga, gt = SR.gradients(V0, lin, ang, torch.tensor(times, dtype=torch.float64), go)
    assert float(gt.abs().max()) > 1e-3                       # (a real gradient, at t = 0 too)
    print(case, "times", SR.rel_max(vt, gt), "closed", SR.rel_max(vc, gt), "V", SR.rel_max(vV[:12], gV[:3].reshape(-1)))
    assert SR.rel_max(vt, gt) < 1e-5
    assert SR.rel_max(vV[:12], gV[:3].reshape(-1)) < 1e-5 and (vV[12:] == 0).all()
    assert SR.rel_max(vl, gl) < 1e-5
    if float(ang.norm()) > 0:
        assert SR.rel_max(va, ga) < 1e-5
    # the dual result is the closed form -<v_out, xi^ V_p> (both float32: a few ulps of the 12-term dot product)
    assert SR.rel_max(vt, vc) < 1e-5
    assert SR.rel_max(vc, gt) < 1e-5


def test_p1_at_t0_is_minus_xi_hat_v(sh, V0):
    lin, ang = torch.tensor([0.1, 0.05, -0.2]), torch.tensor([0.05, -0.08, 0.03])
    go = _cotangent(1)
    _, _, _, vt, _ = _host(sh, V0, lin, ang, [0.0], go)
    want = -float((go[0].double() * (SR.xi_hat(lin, ang) @ V0.double())).sum())
    assert abs(vt[0] - want) < 1e-5 * abs(want) and abs(want) > 1e-3


def test_summed_exposure_gradient_survives_the_cancellation(sh, V0):
    """the case of test_se3_velocity_gradients_survive_the_cancellation_between_sub_poses: symmetric +-5.5 ms with the
    SAME cotangent.  d loss / d exposure = sum_p a_p v_t[p] with a_p = -+1/4 (S = 2): the first-order parts cancel and what
    is left is second order — that test's 2e-4 bar."""
    lin, ang = torch.tensor([0.8, -0.5, 1.1]), torch.tensor([0.9, -1.2, 0.5])
    times = [-0.0055, 0.0055]
    g1 = torch.randn(4, 4, generator=torch.Generator().manual_seed(3))
    g1[3, :] = 0
    go = torch.stack([g1, g1])
    _, _, _, vt, _ = _host(sh, V0, lin, ang, times, go)
    gt = SR.gradients(V0, lin, ang, torch.tensor(np.asarray(times, np.float32).astype(np.float64)), go)[3]
    a = np.array([-0.25, 0.25])
    got, want = float((a * vt.astype(np.float64)).sum()), float((a * gt.numpy()).sum())
    assert abs(want) < 1e-2 * float(gt.abs().max())            # (what is left really is second order)
    print("summed exposure gradient", got, want, abs(got - want) / abs(want))
    assert abs(got - want) < 2e-4 * abs(want)


# ---- ops.subpose_times ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", [(1, 1), (5, 1), (1, 10), (5, 2)])
def test_subpose_times_equals_the_host_schedule_and_differentiates_to_the_coefficients(gs, S, R):
    E, T = 1 / 60, 1 / 37
    want = torch.tensor(gs.subpose_schedule(S, E, R, T)[0], dtype=torch.float32)
    got = gs.subpose_times(S, E, R, T)
    assert got.dtype == torch.float32 and got.shape == (S * R,) and torch.equal(got, want)
    ce, cr = gs.ops.subpose_time_coefficients(S, R)
    assert gs.ops.subpose_time_coefficients(S, R)[0] is ce           # cached per (S, R, device)
    Et, Tt = torch.tensor(E, requires_grad=True), torch.tensor(T, requires_grad=True)
    t = gs.subpose_times(S, Et, R, Tt)
    assert torch.allclose(t, want, rtol=0, atol=1e-9)
    w = torch.randn(S * R, generator=torch.Generator().manual_seed(0))
    (t * w).sum().backward()
    assert torch.allclose(Et.grad, (ce * w).sum()) and torch.allclose(Tt.grad, (cr * w).sum())
    J = torch.autograd.functional.jacobian(lambda e, r: gs.subpose_times(S, e, R, r), (Et.detach(), Tt.detach()))
    assert torch.equal(J[0], ce) and torch.equal(J[1], cr)
    # a float beside a tensor
    assert torch.allclose(gs.subpose_times(S, Et.detach(), R, T), want, rtol=0, atol=1e-9)


# ---- model -----------------------------------------------------------------------------------------------------------
def _model(gs, n=6, num_cameras=4, **shutter):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1, **{k: shutter.pop(k) for k in list(shutter) if k == "motion_model"})
    for k, v in shutter.items():
        setattr(cfg.camera_shutter_optimizer, k, v)
    return gs.SplatfactoDeblurModel(cfg, torch.zeros(n, 3), torch.full((n, 3), math.log(0.01)), torch.ones(n, 4),
                                    torch.zeros(n), torch.zeros(n, 3), torch.zeros(n, 3, 3), num_cameras)


def _cam(gs, i=0, **md):
    return gs.Camera(torch.eye(4)[:3].clone(), 100.0, 100.0, 32.0, 24.0, 64, 48, metadata={"cam_idx": i, **md})


def test_parameter_shapes_per_mode(gs):
    off = _model(gs)
    assert off.exposure_adjustment is None and off.readout_adjustment is None
    assert "camera_shutter_opt" not in gs.training.make_optimizers(off, fused=False)
    assert not [k for k, _ in off.named_parameters() if "adjustment" in k]
    m = _model(gs, exposure="global")
    assert tuple(m.exposure_adjustment.shape) == (1,) and m.readout_adjustment is None
    m = _model(gs, exposure="per_camera", readout="global")
    assert tuple(m.exposure_adjustment.shape) == (4,) and tuple(m.readout_adjustment.shape) == (1,)
    assert float(m.exposure_adjustment.detach().abs().sum()) == 0.0 and float(m.readout_adjustment.detach().abs().sum()) == 0.0
    opts = gs.training.make_optimizers(m, fused=False)
    grp = opts["camera_shutter_opt"].param_groups[0]
    assert grp["eps"] == 1e-15 and grp["lr"] == gs.training.SHUTTER_LR
    assert [p is q for p, q in zip(grp["params"], (m.exposure_adjustment, m.readout_adjustment))] == [True, True]
    m = _model(gs, readout="global")
    assert m.exposure_adjustment is None and tuple(m.readout_adjustment.shape) == (1,)
    assert gs.training.make_optimizers(m, fused=False)["camera_shutter_opt"].param_groups[0]["params"][0] is m.readout_adjustment
    assert [p is m.readout_adjustment for p in gs.training._small_params(m)] == [True]


def test_refusals(gs):
    with pytest.raises(ValueError, match="exposure"):
        _model(gs, exposure="each")
    with pytest.raises(ValueError, match="readout"):
        _model(gs, readout="per_camera")
    with pytest.raises(ValueError, match="se3"):
        _model(gs, motion_model="pixel_velocity", exposure="global")
    with pytest.raises(ValueError, match="se3"):
        _model(gs, motion_model="pixel_velocity", readout="global")
    _model(gs, motion_model="pixel_velocity")                          # off: the pixel-velocity model is as it was
    m = _model(gs, exposure="global", readout="global")
    with pytest.raises(ValueError, match="initial_exposure_time"):
        m._schedule(_cam(gs, rolling_shutter_time=0.01))
    with pytest.raises(ValueError, match="initial_rolling_shutter_time"):
        m._schedule(_cam(gs, exposure_time=0.01))
    # render_step refuses a times gradient outside the SE(3) model before it touches a tensor
    for kw in (dict(motion_model="pixel_velocity"), dict(shared_list=True, motion_model="pixel_velocity"),
               dict(rolling_shutter_time=0.01, motion_model="pixel_velocity")):
        with pytest.raises(ValueError, match="times_grad"):
            gs.render_step(*([None] * 10), 1, 1, 1.0, 1.0, 0.0, 0.0, 8, 8, None, times_grad=True, **kw)


def test_fallback_times_only_where_metadata_is_zero_and_only_when_optimised(gs):
    m = _model(gs, exposure="global", readout="global", initial_exposure_time=0.02, initial_rolling_shutter_time=0.03)
    assert m._base_times(_cam(gs, exposure_time=0.01, rolling_shutter_time=0.005)) == (0.01, 0.005)
    assert m._base_times(_cam(gs)) == (0.02, 0.03)
    assert m._base_times(_cam(gs, exposure_time=0.01)) == (0.01, 0.03)
    S, R, times = m._schedule(_cam(gs))
    assert (S, R) == (5, 10)                                            # decided by the effective starting values
    # exposure only: the readout fallback is NOT used, a missing readout stays 0 and R drops to 1 as always
    m = _model(gs, exposure="global", initial_exposure_time=0.02, initial_rolling_shutter_time=0.03)
    assert m._base_times(_cam(gs)) == (0.02, 0.0)
    assert m._schedule(_cam(gs))[:2] == (5, 1)
    off = _model(gs, initial_exposure_time=0.02, initial_rolling_shutter_time=0.03)
    assert off._base_times(_cam(gs)) == (0.0, 0.0) and off._schedule(_cam(gs))[:2] == (1, 1)


def test_effective_times_and_their_gradients(gs):
    m = _model(gs, exposure="per_camera", readout="global")
    with torch.no_grad():
        m.exposure_adjustment[2] = math.log(2.0)
        m.readout_adjustment[0] = math.log(0.5)
    cam = _cam(gs, 2, exposure_time=0.01, rolling_shutter_time=0.04)
    E, T = m.shutter_times(cam)
    assert E.item() == pytest.approx(0.02, rel=1e-6) and T.item() == pytest.approx(0.02, rel=1e-6)
    assert m.shutter_times(_cam(gs, 1, exposure_time=0.01, rolling_shutter_time=0.04))[0].item() == pytest.approx(0.01)
    # a camera outside [0, num_cameras) or without an index renders with E0
    assert not m.shutter_times(_cam(gs, 9, exposure_time=0.01, rolling_shutter_time=0.04))[0].requires_grad
    S, R, host = m._schedule(cam)
    t = m._times_tensor(cam, S, R, host)
    want = torch.tensor(gs.subpose_schedule(S, 0.02, R, 0.02)[0])
    assert torch.allclose(t, want, rtol=1e-6, atol=1e-9)
    w = torch.randn(S * R, generator=torch.Generator().manual_seed(1))
    (t * w).sum().backward()
    ce, cr = gs.ops.subpose_time_coefficients(S, R)
    g = m.exposure_adjustment.grad
    assert g[2].item() == pytest.approx(float((ce * w).sum()) * 0.02, rel=1e-5) and float(g.abs().sum() - g[2].abs()) == 0.0
    assert m.readout_adjustment.grad[0].item() == pytest.approx(float((cr * w).sum()) * 0.02, rel=1e-5)
    # off: the cached host schedule, the very tensor _const hands out
    off = _model(gs)
    S, R, host = off._schedule(cam)
    assert off._times_tensor(cam, S, R, host) is off._const(host)


def _fake_render(model):
    """a CPU stand-in for the HIP render: an image that depends on the sub-pose times"""
    def render(camera, detach_gaussians=False, return_depth=None):
        S, R, host = model._schedule(camera)
        t = model._times_tensor(camera, S, R, host)
        rgb = (t * t).sum() * 1e3 + torch.zeros(camera.height, camera.width, 3)
        return {"rgb": rgb, "depth": None, "accumulation": None, "background": None}
    return render


def test_eval_camera_step_leaves_the_shutter_estimate_alone(gs, monkeypatch):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1)
    cfg.camera_velocity_optimizer.enabled = True
    cfg.camera_shutter_optimizer.exposure = "per_camera"
    cfg.camera_shutter_optimizer.readout = "global"
    n = 6
    m = gs.SplatfactoDeblurModel(cfg, torch.zeros(n, 3), torch.full((n, 3), math.log(0.01)), torch.ones(n, 4),
                                 torch.zeros(n), torch.zeros(n, 3), torch.zeros(n, 3, 3), 4)
    monkeypatch.setattr(m, "_render", _fake_render(m))
    opts = gs.training.make_optimizers(m, fused=False)
    cam = _cam(gs, 1, exposure_time=0.01, rolling_shutter_time=0.02, is_eval=True)
    gt = torch.zeros(48, 64, 3)
    gs.training.eval_camera_step(m, opts, cam, gt)
    assert m.exposure_adjustment.grad is None and m.readout_adjustment.grad is None
    assert float(m.exposure_adjustment.detach().abs().sum()) == 0.0 and float(m.readout_adjustment.detach().abs().sum()) == 0.0
    assert not opts["camera_shutter_opt"].state
    # ... while a training step moves both (CPU route of train_step through the same stand-in)
    monkeypatch.setattr(m, "get_outputs", lambda camera, **kw: m._render(camera))
    gs.training.train_step(m, opts, cam, gt)
    assert float(m.exposure_adjustment[1].detach().abs()) > 0 and float(m.readout_adjustment.detach().abs().sum()) > 0
    assert float(m.exposure_adjustment.detach().abs().sum() - m.exposure_adjustment[1].abs()) == 0.0


# ---- checkpoints -----------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_the_optimizer_on_is_bit_equal(gs, tmp_path):
    C = gs.checkpoint
    m = _model(gs, exposure="per_camera", readout="global", initial_exposure_time=0.02)
    opts = gs.training.make_optimizers(m, fused=False)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        gs.training.optimizers_step(opts.values())
    assert float(m.exposure_adjustment.detach().abs().min()) > 0
    C.save_checkpoint(tmp_path / "on.pt", m, opts)
    raw = torch.load(tmp_path / "on.pt", weights_only=True)
    assert raw["version"] == 1
    assert raw["model"]["config"]["camera_shutter_optimizer"] == {
        "exposure": "per_camera", "readout": "global", "initial_exposure_time": 0.02, "initial_rolling_shutter_time": None}
    assert torch.equal(raw["model"]["exposure_adjustment"], m.exposure_adjustment.detach())
    assert isinstance(raw["optimizers"]["groups"]["camera_shutter_opt"]["step"], list)
    ck = C.load_checkpoint(tmp_path / "on.pt", "cpu")
    assert ck.model.config == m.config
    p0, p1 = dict(m.named_parameters()), dict(ck.model.named_parameters())
    assert set(p0) == set(p1) and {"exposure_adjustment", "readout_adjustment"} <= set(p0)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    o0, o1 = opts["camera_shutter_opt"], ck.optimizers["camera_shutter_opt"]
    for q0, q1 in zip(o0.param_groups[0]["params"], o1.param_groups[0]["params"]):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(torch.as_tensor(o0.state[q0][key]), torch.as_tensor(o1.state[q1][key])), key
    # and into an existing model of the same config
    again = _model(gs, exposure="per_camera", readout="global", initial_exposure_time=0.02)
    C.load_checkpoint(tmp_path / "on.pt", into=again)
    assert torch.equal(again.exposure_adjustment, m.exposure_adjustment)
    assert torch.equal(again.readout_adjustment, m.readout_adjustment)


def test_checkpoint_with_the_optimizer_off_has_the_key_set_it_always_had(gs, tmp_path):
    C = gs.checkpoint
    m = _model(gs)
    opts = gs.training.make_optimizers(m, fused=False)
    C.save_checkpoint(tmp_path / "off.pt", m, opts)
    raw = torch.load(tmp_path / "off.pt", weights_only=True)
    assert set(raw["model"]) == {"config", "num_cameras", "step", "params", "background_param", "pose_adjustment",
                                 "velocity_adjustment", "bilateral_grids"}
    assert "camera_shutter_opt" not in raw["optimizers"]["groups"]
    # a file written before the feature: no config block for it, no keys — loads as "off"
    del raw["model"]["config"]["camera_shutter_optimizer"]
    torch.save(raw, tmp_path / "old.pt")
    ck = C.load_checkpoint(tmp_path / "old.pt", "cpu")
    assert ck.model.exposure_adjustment is None and ck.model.readout_adjustment is None
    assert ck.model.config.camera_shutter_optimizer == gs.CameraShutterOptimizerConfig()
    assert "camera_shutter_opt" not in ck.optimizers
