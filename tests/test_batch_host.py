"""Batched cameras (ops.render_batch, model.get_outputs_batch, DensifyState with [B,N,2]): the host-side logic that
needs no GPU — argument validation before anything is launched, the model's grouping of mixed-intrinsics camera lists,
and the densification statistics of a batch."""
import math

import pytest
import torch


def _gauss(n=8):
    return (torch.zeros(n, 3), torch.ones(n, 3), torch.ones(n, 4), torch.ones(n), torch.zeros(n, 16, 3))


def _call(gs, B, S, R, H, W, **kw):
    vm = kw.pop("viewmats", None)
    if vm is None:
        vm = torch.eye(4).expand(B, S * R, 4, 4).contiguous()
    return gs.render_batch(*_gauss(), vm, None, S, R, 100.0, 100.0, W / 2, H / 2, H, W, **kw)


def test_render_batch_rejects_bad_viewmat_shapes(gs):
    with pytest.raises(ValueError, match=r"viewmats must be \[B,10,4,4\]"):
        _call(gs, 2, 5, 2, 64, 64, viewmats=torch.eye(4).expand(2, 5, 4, 4))
    with pytest.raises(ValueError, match="viewmats must be"):
        _call(gs, 2, 5, 1, 64, 64, viewmats=torch.eye(4).expand(10, 4, 4))


def test_render_batch_rejects_more_than_256_subposes(gs):
    with pytest.raises(ValueError, match="at most 256"):
        _call(gs, 6, 5, 10, 64, 64)                     # 300 sub-poses
    gs.ops.check_batch(5, 5, 10, 64, 64)                # 250: allowed


def test_render_batch_rejects_32_bit_pixel_overflow(gs):
    # 4 cameras x 5 samples x 16384^2 >= 2^31, and the frame's own bound (2^30) is named in the message
    with pytest.raises(ValueError, match=r"2\^30"):
        _call(gs, 4, 5, 1, 16384, 16384)
    with pytest.raises(ValueError, match=r"2\^30"):
        gs.ops.check_batch(26, 5, 1, 2160, 3840)
    gs.ops.check_batch(2, 5, 1, 2160, 3840)             # 10 camera-samples at 4K fit


def test_render_batch_rejects_pixel_velocity_and_shared_list(gs):
    with pytest.raises(NotImplementedError, match="pixel-velocity"):
        _call(gs, 2, 3, 1, 32, 32, times=torch.zeros(3))
    with pytest.raises(NotImplementedError, match="shared-list"):
        _call(gs, 2, 3, 1, 32, 32, shared_list=True)


def test_render_batch_rejects_wrong_xy_grad_shape(gs):
    with pytest.raises(ValueError, match=r"\[B,N,2\]"):
        _call(gs, 2, 3, 1, 32, 32, xy_grad_out=torch.zeros(8, 2))


def test_render_batch_refuses_the_python_frame_backend(gs, monkeypatch):
    class Twin:
        def native_ok(self):
            return False
    monkeypatch.setattr(gs.ops, "frame_backend", Twin())
    with pytest.raises(NotImplementedError, match="frame path"):
        _call(gs, 2, 3, 1, 32, 32)


def _model(gs, n=6):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=1)
    return gs.SplatfactoDeblurModel(cfg, torch.zeros(n, 3), torch.full((n, 3), math.log(0.01)), torch.ones(n, 4),
                                    torch.zeros(n), torch.zeros(n, 3), torch.zeros(n, 3, 3), 8)


def _cam(gs, i, fx=100.0, W=64, H=48, exposure=0.01):
    c2w = torch.eye(4)[:3].clone()
    c2w[0, 3] = float(i)
    return gs.Camera(c2w, fx, fx, W / 2, H / 2, W, H, metadata={"cam_idx": i, "exposure_time": exposure})


def test_model_groups_mixed_intrinsics_in_input_order(gs, monkeypatch):
    model = _model(gs)
    model.eval()
    calls = []

    def stand_in(items, return_depth, detach_gaussians=False):
        # one "frame" per group: rgb of camera k = its cam_idx / 10 everywhere, radii / xy marked the same way
        calls.append([int(c.metadata["cam_idx"]) for c, _, _, _ in items])
        B = len(items)
        cam0, S, R, _ = items[0]
        H, W = cam0.height, cam0.width
        idx = torch.tensor([float(c.metadata["cam_idx"]) for c, _, _, _ in items])
        rgb = (idx / 10)[:, None, None, None].expand(B, H, W, 3).clone()       # (get_outputs clamps at 1)
        alphas = torch.ones(B, S, H, W)
        radii = idx[:, None, None].expand(B, S * R, model.num_points).to(torch.int32).clone()
        res = (rgb, alphas, radii, torch.ones(B, S, H, W)) if return_depth else (rgb, alphas, radii)
        return res, None, torch.zeros(3)

    monkeypatch.setattr(model, "_render_group", stand_in)
    cams = [_cam(gs, 0), _cam(gs, 1, fx=90.0), _cam(gs, 2), _cam(gs, 3, fx=90.0), _cam(gs, 4, exposure=0.0),
            _cam(gs, 5)]
    out = model.get_outputs_batch(cams)
    # groups: fx=100 (0, 2, 5), fx=90 (1, 3), one blur sample (4) — in the order of each group's first camera
    assert calls == [[0, 2, 5], [1, 3], [4]]
    assert out["rgb"].shape == (6, 48, 64, 3)
    assert [round(10 * float(out["rgb"][j, 0, 0, 0])) for j in range(6)] == [0, 1, 2, 3, 4, 5]       # input order
    assert out["depth"].shape == (6, 48, 64, 1) and out["accumulation"].shape == (6, 48, 64, 1)
    assert [int(r.reshape(-1)[0]) for r in model.radii] == [0, 1, 2, 3, 4, 5]


def test_model_batch_of_mixed_sizes_returns_lists(gs, monkeypatch):
    model = _model(gs)
    model.eval()

    def stand_in(items, return_depth, detach_gaussians=False):
        B = len(items)
        cam0, S, R, _ = items[0]
        res = (torch.zeros(B, cam0.height, cam0.width, 3), torch.ones(B, S, cam0.height, cam0.width),
               torch.zeros(B, S * R, model.num_points, dtype=torch.int32))
        return res + ((torch.ones(B, S, cam0.height, cam0.width),) if return_depth else ()), None, torch.zeros(3)

    monkeypatch.setattr(model, "_render_group", stand_in)
    out = model.get_outputs_batch([_cam(gs, 0), _cam(gs, 1, W=32, H=24), _cam(gs, 2)])
    assert [tuple(t.shape) for t in out["rgb"]] == [(48, 64, 3), (24, 32, 3), (48, 64, 3)]


def test_model_batch_rejects_pixel_velocity_model(gs):
    model = _model(gs)
    model.config.motion_model = "pixel_velocity"
    with pytest.raises(NotImplementedError, match="SE\\(3\\)"):
        model.get_outputs_batch([_cam(gs, 0), _cam(gs, 1)])


def test_densify_batch_equals_single_camera_updates(gs):
    g = torch.Generator().manual_seed(3)
    B, P, N = 4, 6, 50
    radii = torch.randint(0, 3, (B, P, N), generator=g, dtype=torch.int32) * torch.randint(0, 20, (B, 1, N), generator=g,
                                                                                             dtype=torch.int32)
    xy = torch.randn(B, N, 2, generator=g)
    a = gs.densify.DensifyState(N, "cpu")
    a.after_backward(radii, xy, 64, 48)
    b = gs.densify.DensifyState(N, "cpu")
    for k in range(B):
        b.after_backward(radii[k], xy[k], 64, 48)
    assert torch.equal(a.xys_grad_norm, b.xys_grad_norm)
    assert torch.equal(a.vis_counts, b.vis_counts)
    assert torch.equal(a.max_2Dsize, b.max_2Dsize)
    assert a.size == b.size == (64, 48)
    # each camera is one observation: a Gaussian visible to every camera counts B
    vis = (radii > 0).any(dim=1).sum(dim=0).to(torch.float32)
    assert torch.equal(a.vis_counts, vis)
    # per-camera lists (several frames of one batch) count the same way
    c = gs.densify.DensifyState(N, "cpu")
    c.after_backward(list(radii.unbind(0)), list(xy.unbind(0)), 64, 48)
    assert torch.equal(c.xys_grad_norm, a.xys_grad_norm) and torch.equal(c.vis_counts, a.vis_counts)
