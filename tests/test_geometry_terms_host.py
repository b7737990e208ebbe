"""train_step's list of geometry terms (train_step.geometry_terms) on the CPU model of the depth-prior and normal host tests:
which terms every keyword combination gives and in which order, how each route consumes the list, and that the value logged
is the image loss plus the public ops' values; and the autograd Function the losses on the sums share (_sums.SumsLoss)."""
import itertools

import pytest
import torch

import depthprior_reference as DR
import normal_reference as NR
from test_normals_host import _trainable

COMBOS = list(itertools.product(("none", "metric", "pearson"), (False, True), (False, True)))


def _keywords(depth, prior_on, smooth_on, gt_depth, gt_normal):
    kw = {}
    if depth != "none":
        kw.update(gt_depth=gt_depth, depth_lambda=0.5, depth_loss=None if depth == "metric" else depth)
    if prior_on:
        kw.update(gt_normal=gt_normal, normal_lambda=0.5)
    if smooth_on:
        kw.update(normal_smooth_lambda=0.3, normal_edge_beta=2.0)
    return kw


def _names(depth, prior_on, smooth_on):
    return (["depth_loss"] if depth != "none" else []) + (["normal_loss"] if prior_on or smooth_on else [])


def _term_values_on_map(gs, depth, prior_on, smooth_on, out, cam, img, dprior, nprior, hole, H, W):
    """the public ops' values on a rendered depth map, in the list's order"""
    T = gs.training
    m = hole.reshape(1, H, W)
    acc = out["depth"].detach().reshape(1, H, W) * m
    vals = []
    if depth == "metric":
        vals.append(float(T.depth_loss(out["depth"].detach(), dprior, 0.5)))
    elif depth != "none":
        vals.append(float(gs.depth_prior_loss(acc, m, dprior.reshape(H, W), depth, "depth", 0.5)))
    if prior_on or smooth_on:
        vals.append(float(gs.normal_loss(acc, m, (cam.fx, cam.fy, cam.cx, cam.cy), nprior if prior_on else None,
                                         img if smooth_on else None, 0.5 if prior_on else 0.0, 0.3 if smooth_on else 0.0,
                                         2.0 if smooth_on else 0.0)))
    return vals


@pytest.mark.parametrize("depth,prior_on,smooth_on", COMBOS, ids=lambda v: str(v))
def test_term_list_and_what_every_route_does_with_it(gs, monkeypatch, depth, prior_on, smooth_on):
    T = gs.training
    model, cam, nprior, base, hole, H, W = _trainable(gs)
    g = torch.Generator().manual_seed(21)
    img = torch.rand(H, W, 3, generator=g)
    dprior = (0.37 * base + 1.9 + 0.3 * torch.rand(H, W, generator=g))[..., None]
    dprior[:, 3] = 0.0
    kw = _keywords(depth, prior_on, smooth_on, dprior, nprior)
    names = _names(depth, prior_on, smooth_on)

    # the list: names and order, and nothing for a camera whose map is missing
    def build(gt_depth, gt_normal):
        k = _keywords(depth, prior_on, smooth_on, gt_depth, gt_normal)
        return T.geometry_terms(model, cam, img, k.get("gt_depth"), k.get("depth_lambda", 0.0), k.get("depth_loss"), "depth",
                                k.get("gt_normal"), k.get("normal_lambda", 0.0), k.get("normal_smooth_lambda", 0.0),
                                k.get("normal_edge_beta", 0.0))
    assert [t.name for t in build(dprior, nprior)] == names
    assert [t.name for t in build(None, None)] == (["normal_loss"] if smooth_on else [])

    # the autograd route: image loss + the ops on the rendered depth map, in the list's order
    out = model.get_outputs(cam)
    image_term = float(T.image_loss_torch(out["rgb"], img, 0.0).detach())
    vals = _term_values_on_map(gs, depth, prior_on, smooth_on, out, cam, img, dprior, nprior, hole, H, W)
    assert len(vals) == len(names)
    h = T.train_step(model, T.make_optimizers(model), cam, img, 0.0, **kw)
    assert h["loss"] == pytest.approx(image_term + sum(vals), abs=1e-6)

    # the batch route, with every map and with a camera that has none: the mean of the per-camera sums
    none_vals = _term_values_on_map(gs, "none", False, smooth_on, out, cam, img, dprior, nprior, hole, H, W)
    for maps, second in ((lambda t: [t, t], vals), (lambda t: [t, None], none_vals)):
        model, cam, _, _, _, _, _ = _trainable(gs)
        single = model.get_outputs
        model.get_outputs_batch = lambda cams, **k: {key: torch.stack([single(c)[key] for c in cams])
                                                     for key in ("rgb", "depth", "accumulation")}
        hb = T.train_step(model, T.make_optimizers(model), [cam, cam], [img, img], 0.0,
                          **_keywords(depth, prior_on, smooth_on, maps(dprior), maps(nprior)))
        assert hb["loss"] == pytest.approx(image_term + (sum(vals) + sum(second)) / 2, abs=1e-6)

    # the one-call route with a stand-in frame: which keyword travels, and what the callable returns and logs
    model, cam, _, _, _, _, _ = _trainable(gs)
    monkeypatch.setattr(T, "one_call_route", lambda m: True)
    monkeypatch.setattr(gs.fused, "image_loss_with_grad", lambda rgb, gt, lam: (torch.tensor(0.25), torch.zeros_like(rgb), None))
    S = 3
    alphas = (torch.rand(S, H, W, generator=g) * 0.9 + 0.1) * hole.reshape(1, H, W)
    depth_acc = alphas * (base + 0.3 * torch.rand(H, W, generator=g))
    depth_map = torch.full((H, W, 1), 3.0)
    seen = {}

    def stand_in(camera, grad_image, grad_depth=None, grad_depth_sums=None):
        seen["keywords"] = (grad_depth is not None, grad_depth_sums is not None)
        grad_image(torch.full((H, W, 3), 0.5))
        if grad_depth is not None:
            seen["grads"] = grad_depth(depth_map.clone(), hole)
        if grad_depth_sums is not None:
            seen["grads"] = grad_depth_sums(depth_acc, alphas)
        for p in model.gauss_params().values():
            p.grad = torch.zeros_like(p)
        model.radii = torch.ones(1, model.num_points, dtype=torch.int32)
        return torch.full((H, W, 3), 0.5)

    model.render_and_backward = stand_in
    h = T.train_step(model, T.make_optimizers(model, fused=False), cam, img, 0.2, **kw)
    lone_metric = depth == "metric" and not (prior_on or smooth_on)
    assert seen["keywords"] == ((False, False) if not names else (True, False) if lone_metric else (False, True))
    want, grads = [], []
    if lone_metric:
        want.append(float(T.depth_loss(depth_map, dprior, 0.5)))
    elif depth == "metric":
        a, b = depth_acc.clone().requires_grad_(True), alphas.clone().requires_grad_(True)
        ml = T.depth_loss(gs.model.expected_depth(a, b), dprior, 0.5)
        ml.backward()
        want.append(float(ml.detach()))
        grads.append((a.grad, b.grad))
    elif depth != "none":
        dl, dvd, dva = gs.depth_prior_loss_with_grad(depth_acc, alphas, dprior.reshape(H, W), depth, "depth", 0.5)
        want.append(float(dl))
        grads.append((dvd, dva))
    if prior_on or smooth_on:
        nl, nvd, nva = gs.normal_loss_with_grad(depth_acc, alphas, (cam.fx, cam.fy, cam.cx, cam.cy), nprior if prior_on else None,
                                                img if smooth_on else None, 0.5 if prior_on else 0.0,
                                                0.3 if smooth_on else 0.0, 2.0 if smooth_on else 0.0)
        want.append(float(nl))
        grads.append((nvd, nva))
    assert h["loss"] == pytest.approx(0.25 + sum(want), abs=1e-6)
    if grads:
        for k in (0, 1):
            total = grads[0][k] if len(grads) == 1 else grads[0][k] + grads[1][k]
            assert torch.allclose(seen["grads"][k], total, rtol=0, atol=1e-9)
            if depth != "metric":
                assert torch.equal(seen["grads"][k], total)


def test_shared_autograd_function_scales_the_forward_gradients(gs):
    """_sums.SumsLoss around each op's with-grad form: the .grad the ops' own CPU autograd tests pin (test_depthprior_host,
    test_normals_host: test_autograd_function_on_the_cpu), for a [B] and for a scalar upstream gradient"""
    F = gs._sums.SumsLoss
    acc, al, pr, _ = (torch.from_numpy(t) if hasattr(t, "dtype") else t for t in DR.make_batch(2, 3, 9, 11, "depth", seed=2))
    nacc, nal, K, nprior, guide = (torch.from_numpy(t) for t in NR.make_batch(2, 3, 9, 11, seed=2))
    cases = [(gs.depth_prior_loss_with_grad, gs.depth_prior_loss, acc, al, lambda b: (pr[b], "pearson", "depth", 0.7, 0.0)),
             (gs.normal_loss_with_grad, gs.normal_loss, nacc, nal, lambda b: (K[b], nprior[b], guide[b], 0.7, 0.4, 2.0, 0.0))]
    for with_grad, public, acc, al, const in cases:
        every = slice(None)
        loss, vd, va = with_grad(acc, al, *const(every))
        a, b = acc.clone().requires_grad_(True), al.clone().requires_grad_(True)
        out = F.apply(with_grad, a, b, *const(every))
        assert torch.equal(out.detach(), loss) and torch.equal(out.detach(), public(acc, al, *const(every)))
        (out * torch.tensor([1.0, 0.5])).sum().backward()
        assert torch.equal(a.grad[0], vd[0]) and torch.equal(a.grad[1], vd[1] * 0.5)
        assert torch.equal(b.grad[0], va[0]) and torch.equal(b.grad[1], va[1] * 0.5)
        # a scalar loss and a scalar upstream gradient; only depth_acc asks for a gradient
        a1 = acc[1].clone().requires_grad_(True)
        one = F.apply(with_grad, a1, al[1], *const(1))
        assert one.shape == () and torch.equal(one.detach(), loss[1])
        (one * 0.5).backward()
        assert torch.equal(a1.grad, vd[1] * 0.5)
