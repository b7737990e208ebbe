"""Gradient routing of the frame node on the CPU: ops.frame_forward / frame_backward and ops.subpose_forward /
subpose_backward are replaced by stand-ins that return correctly shaped outputs and, per gradient NAME, a tensor filled
with that name's constant.  Whatever sits between the public entry points and those functions — the autograd wrappers,
the order of the node's inputs, render_step's dictionary — must hand every tensor exactly its own constant."""
from types import SimpleNamespace

import pytest
import torch

N, H, W, S, R = 8, 32, 32, 2, 1
FRAME = dict(means=1.0, scales=2.0, quats=3.0, opacities=4.0, sh=5.0, sh_rest=6.0, viewmats=7.0, background=8.0,
             lin_vel=9.0, ang_vel=10.0)
SUBPOSE = dict(viewmat=11.0, lin_vel=12.0, ang_vel=13.0, times=14.0)
GAUSS = ("means", "scales", "quats", "opacities", "sh", "sh_rest")
CAM = (30.0, 30.0, 16.0, 16.0, H, W)


@pytest.fixture()
def ops(gs, monkeypatch):
    from gsdeblur_amd import ops
    seen = SimpleNamespace(want=[], want_times=[])

    def frame_forward(spec, means, scales, quats, opacities, sh, sh_rest=None, viewmats=None, background=None,
                      lin_vel=None, ang_vel=None, *, want=frozenset(), times=None, xy_grad_out=None, xy_absgrad_out=None,
                      hints=None):
        seen.want.append(want)
        B, P = spec.cameras, (1 if spec.shared_list else spec.S * spec.R)
        img = (spec.S, H, W, 3) if spec.gamma is None else ((H, W, 3) if B == 1 else (B, H, W, 3))
        given = dict(means=means, scales=scales, quats=quats, opacities=opacities, sh=sh, sh_rest=sh_rest,
                     viewmats=viewmats, background=background, lin_vel=lin_vel, ang_vel=ang_vel)
        state = SimpleNamespace(want=want, shapes={k: tuple(v.shape) for k, v in given.items() if v is not None})
        return ((torch.zeros(img), torch.zeros(spec.S, H, W) if spec.return_alpha else None,
                 torch.zeros(P, N, dtype=torch.int32), None), state,
                ops.FrameTensors._make([None] * len(ops.FrameTensors._fields)))

    def frame_backward(state, tensors, v_img, v_alpha, v_depth=None):
        assert isinstance(tensors, ops.FrameTensors)
        off = {"viewmats": "viewmats", "background": "background", "lin_vel": "twist", "ang_vel": "twist"}
        return ops.FrameGrads(**{k: torch.full(shape, FRAME[k]) for k, shape in state.shapes.items()
                                 if off.get(k, "gaussians") in state.want or k in GAUSS})

    def subpose_forward(viewmat, lin_vel, ang_vel, times):
        return torch.zeros(times.numel(), 4, 4), (viewmat, lin_vel, ang_vel, times)

    def subpose_backward(saved, v_out, want_times):
        seen.want_times.append(want_times)
        assert torch.equal(v_out, torch.full((saved[3].numel(), 4, 4), FRAME["viewmats"]))
        return (torch.full((4, 4), SUBPOSE["viewmat"]), torch.full((3,), SUBPOSE["lin_vel"]),
                torch.full((3,), SUBPOSE["ang_vel"]), torch.full(saved[3].shape, SUBPOSE["times"]) if want_times else None)

    for fn in (frame_forward, frame_backward, subpose_forward, subpose_backward):
        monkeypatch.setattr(ops, fn.__name__, fn)
    ops.seen = seen
    yield ops
    del ops.seen


def leaves(split, grad=True):
    t = dict(means=torch.zeros(N, 3), scales=torch.ones(N, 3), quats=torch.ones(N, 4), opacities=torch.ones(N),
             sh=torch.zeros(N, 3) if split else torch.zeros(N, 16, 3), background=torch.zeros(3), viewmat=torch.eye(4),
             lin_vel=torch.zeros(3), ang_vel=torch.zeros(3), times=torch.linspace(-0.01, 0.01, S * R))
    if split:
        t["sh_rest"] = torch.zeros(N, 15, 3)
    return {k: v.requires_grad_(grad) for k, v in t.items()}


def gauss_args(t):
    return t["means"], t["scales"], t["quats"], t["opacities"], t["sh"]


def check_grads(t, want):
    for k, v in t.items():
        if k in want:
            assert v.grad is not None and torch.equal(v.grad, torch.full(v.shape, want[k])), k
        else:
            assert v.grad is None, k


def camera():
    t = dict(viewmat=torch.eye(4), lin_vel=torch.zeros(3), ang_vel=torch.zeros(3), times=torch.linspace(-0.01, 0.01, S * R))
    return {k: v.requires_grad_(True) for k, v in t.items()}


# render_batch renders SE(3) sub-poses only (tests/test_batch_host.py): no pixel-velocity case for it
ENTRIES = [(e, f) for e in ("render_subposes", "render_combined", "render_batch_1", "render_batch_2")
           for f in ("viewmats", "se3", "pixel_velocity") if not (e.startswith("render_batch") and f == "pixel_velocity")]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("entry, form", ENTRIES)
def test_every_input_gets_its_own_gradient(ops, entry, form, split):
    """(a): through the public entry points; `viewmats` = a leaf [(B,)P,4,4], `se3` = through subpose_viewmats (one set
    of camera leaves per camera of a batch), `pixel_velocity` = viewmat, twist and times handed to the frame itself"""
    batch = int(entry[-1]) if entry.startswith("render_batch") else 0
    t = {k: v for k, v in leaves(split).items() if k in GAUSS + ("background",)}
    want = {k: FRAME[k] for k in t}
    cams = [camera() for _ in range(max(1, batch))]
    kw = dict(sh_rest=t.get("sh_rest"))
    if form == "pixel_velocity":
        vms = cams[0]["viewmat"]
        kw.update(lin_vel=cams[0]["lin_vel"], ang_vel=cams[0]["ang_vel"], times=cams[0]["times"])
        cam_want = dict(viewmat=FRAME["viewmats"], lin_vel=FRAME["lin_vel"], ang_vel=FRAME["ang_vel"])   # times: none
    elif form == "se3":
        vms = torch.stack([ops.subpose_viewmats(c["viewmat"], c["lin_vel"], c["ang_vel"], c["times"]) for c in cams])
        vms, cam_want = (vms if batch else vms[0]), SUBPOSE
    else:
        shape = (batch, S * R, 4, 4) if batch else (S * R, 4, 4)
        vms = t["viewmats"] = torch.eye(4).expand(shape).clone().requires_grad_(True)
        want["viewmats"], cam_want = FRAME["viewmats"], {}
    if batch:
        rgb, alphas, radii = ops.render_batch(*gauss_args(t), vms, t["background"], S, R, *CAM, **kw)
        assert rgb.shape == (batch, H, W, 3) and alphas.shape == (batch, S, H, W) and radii.shape == (batch, S * R, N)
    else:
        rgb, alphas, radii = getattr(ops, entry)(*gauss_args(t), vms, t["background"], S, R, *CAM, **kw)
        assert rgb.shape == ((S, H, W, 3) if entry == "render_subposes" else (H, W, 3)) and radii.shape == (S * R, N)
    assert not radii.requires_grad
    (rgb.sum() + alphas.sum()).backward()
    check_grads(t, want)
    for c in cams:
        check_grads(c, cam_want)
    assert ops.seen.want_times == ([True] * len(cams) if form == "se3" else [])
    assert ops.seen.want == [frozenset(["gaussians", "viewmats", "background"] + (["sh_rest"] if split else [])
                                       + (["twist"] if form == "pixel_velocity" else []))]


@pytest.mark.parametrize("needs, want", [
    ((), ()), (("means",), ("gaussians",)), (("sh",), ("gaussians",)), (("sh_rest",), ("sh_rest",)),
    (("viewmat",), ("viewmats",)), (("background",), ("background",)), (("lin_vel",), ("twist",)),
    (("ang_vel", "opacities"), ("twist", "gaussians")), (("times",), ())])
def test_wanted_gradients_follow_requires_grad(ops, needs, want):
    """(c): the pixel-velocity form takes every differentiable input directly"""
    t = leaves(True, grad=False)
    for k in needs:
        t[k].requires_grad_(True)
    rgb, _, _ = ops.render_combined(*gauss_args(t), t["viewmat"], t["background"], S, R, *CAM, sh_rest=t["sh_rest"],
                                    lin_vel=t["lin_vel"], ang_vel=t["ang_vel"], times=t["times"])
    assert ops.seen.want == [frozenset(want)]
    assert rgb.requires_grad == bool(want)
    if want:
        rgb.sum().backward()
        names = dict(FRAME, viewmat=FRAME["viewmats"])
        check_grads(t, {k: names[k] for k in needs})


# times_grad is an SE(3) form (tests/test_shutter_host.py)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("background_grad", [False, True])
@pytest.mark.parametrize("camera_grads", [False, True])
@pytest.mark.parametrize("model, times_grad", [("se3", False), ("se3", True), ("pixel_velocity", False)])
def test_render_step_fills_its_dictionary_by_name(gs, ops, model, camera_grads, background_grad, split, times_grad):
    """(b)"""
    pixvel = model == "pixel_velocity"
    t = leaves(split, grad=False)
    rgb, g, radii = gs.render_step(*gauss_args(t), t["viewmat"], t["lin_vel"], t["ang_vel"], t["times"], t["background"],
                                   S, R, *CAM, torch.ones(H, W, 3), sh_rest=t.get("sh_rest"), motion_model=model,
                                   camera_grads=camera_grads, background_grad=background_grad, times_grad=times_grad)
    assert rgb.shape == (H, W, 3) and radii.shape == (S * R, N)
    want = {k: FRAME[k] for k in GAUSS if k in t}
    if background_grad:
        want["background"] = FRAME["background"]
    if camera_grads:
        cam = dict(viewmat=FRAME["viewmats"], lin_vel=FRAME["lin_vel"], ang_vel=FRAME["ang_vel"]) if pixvel else SUBPOSE
        want.update({k: cam[k] for k in ("viewmat", "lin_vel", "ang_vel")})
    if times_grad:
        want["times"] = SUBPOSE["times"]
    keys = {"means", "scales", "quats", "opacities", "sh", "sh_rest", "viewmat", "lin_vel", "ang_vel", "background"}
    assert set(g) == keys | ({"times"} if times_grad else set())
    for k, v in g.items():
        if k in want:
            assert torch.equal(v, torch.full(t[k].shape, want[k])), k
        else:
            assert v is None, k
    assert ops.seen.want == [frozenset(["gaussians"] + (["sh_rest"] if split else [])
                                       + (["viewmats"] if camera_grads or times_grad else [])
                                       + (["twist"] if camera_grads and pixvel else [])
                                       + (["background"] if background_grad else []))]
    assert ops.seen.want_times == ([times_grad] if (camera_grads or times_grad) and not pixvel else [])
