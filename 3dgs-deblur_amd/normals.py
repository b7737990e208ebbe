"""Normals from the rendered depth, and the two losses on them: the depth-normal regularisers of DN-Splatter and of the
2DGS / GOF family (recollected, none of them is part of the reference tree).

``depth_normals`` back-projects every pixel's depth with the camera's intrinsics and takes the cross product of the two
central differences: a camera-frame unit vector (x right, y down, z forward) that faces the camera, (0, 0, 0) where a
pixel, one of its four axis neighbours or the cross product has no value.  ``normal_loss`` pulls those normals towards a
monocular normal prior where one exists (``prior_weight * mean(1 - n.m)``) and towards their neighbours
(``smooth_weight * mean over the adjacent pairs of g (1 - n_p.n_q)``, ``g = exp(-edge_beta * mean |dI|)`` of a guide image:
smooth where the picture is).  Both terms are the cosine form, which has no kink; an L1 on the components is not offered
(DESIGN 5.15).

The op starts from the compositor's raw per-sample sums (csrc/normal_math.h states every operation): depth_acc and alphas
[S,H,W], ``d`` and ``a`` their sample means as in depthprior, ``z = d / a`` where ``a > min_alpha and d > 0``.  A rendered
depth map goes in as ``depth_acc = depth * m``, ``alphas = m`` for ``m = (accumulation > 0)``, one sample.  Per-pixel
values are float32 with every operation rounded, the sums and the gradient chain float64.

On HIP tensors the kernels of csrc/normals.hip are the only route (``gs_depth_normals``: one launch; ``gs_normal_loss``:
two launches, no atomics, nothing read back, bit-identical from run to run and independent of the rest of the batch); CPU
tensors take ``depth_normals_torch`` / ``normal_loss_torch``, the same operations as torch ops."""
from __future__ import annotations

import ctypes
import functools
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _sums
from ._sums import MAX_ELEMS, MAX_PLANES  # noqa: F401  (the limits of every loss on the sums)

STATS = 6                            # csrc/normal_math.h kStats: normals, Np, sum(1 - n.m), Ns, sum g (1 - n_p.n_q), sum g
MIN_L2 = 1e-30                       # kMinL2


def _check(depth_acc, alphas, intrins, prior=None, guide=None, prior_weight=1.0, smooth_weight=0.0, edge_beta=0.0,
           min_alpha=0.0) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor], Optional[Tensor], bool]:
    """-> (depth_acc [B,S,H,W], alphas, intrins float32 [B,4] on the CPU, prior [B,H,W,3] or None, guide or None, single),
    detached; ValueError for anything else"""
    depth_acc, alphas, single = _sums.check_sums("the normal ops support", depth_acc, alphas, prior=prior, guide=guide)
    B, S, H, W = (int(s) for s in depth_acc.shape)
    images = []
    for name, t in (("prior", prior), ("guide", guide)):
        if t is not None:
            want = (H, W, 3) if single else (B, H, W, 3)
            if tuple(t.shape) != want:
                raise ValueError(f"{name} must be {list(want)}, got {tuple(t.shape)}")
            t = t.detach()
            t = t[None] if single else t
        images.append(t)
    K = torch.as_tensor(intrins, dtype=torch.float32).detach().cpu()
    if tuple(K.shape) == (4,):
        K = K[None].expand(B, 4)
    if tuple(K.shape) != (B, 4):
        raise ValueError(f"intrins must be fx, fy, cx, cy or [{B},4], got {tuple(K.shape)}")
    if not bool(torch.isfinite(K).all()) or not bool((K[:, :2] > 0).all()):
        raise ValueError("intrins must be finite with fx, fy > 0")
    for name, w in (("prior_weight", prior_weight), ("smooth_weight", smooth_weight), ("edge_beta", edge_beta),
                    ("min_alpha", min_alpha)):
        if not (float(w) >= 0.0 and math.isfinite(float(w))):
            raise ValueError(f"{name} must be a finite number >= 0, got {w}")
    return depth_acc, alphas, K.contiguous(), images[0], images[1], single


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=256)
def _device_intrins_cached(values: tuple, B: int, device: str) -> Tensor:
    return torch.tensor(values, dtype=torch.float32).reshape(B, 4).to(device)


def _device_intrins(K: Tensor, dev) -> Tensor:
    """the [B,4] intrinsics on the device; kept per (values, device), so that a trainer's cameras cost one small copy each
    and not one host-blocking copy per step"""
    return _device_intrins_cached(tuple(K.reshape(-1).tolist()), int(K.shape[0]), str(dev))


def depth_normals_hip(depth_acc: Tensor, alphas: Tensor, intrins, min_alpha: float = 0.0) -> Tensor:
    """gs_depth_normals on GPU tensors: depth_acc, alphas [B,S,H,W], intrins [B,4] -> normals [B,H,W,3]"""
    from . import _lib
    _sums.check_hip(depth_acc)
    depth_acc, alphas, K, _, _, _ = _check(depth_acc, alphas, intrins, min_alpha=min_alpha)
    depth_acc, alphas = depth_acc.contiguous(), alphas.contiguous()
    B, S, H, W = (int(s) for s in depth_acc.shape)
    dev = depth_acc.device
    normals = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    if B == 0:
        return normals
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(dev):
        K = _device_intrins(K, dev)
        _lib.check(lib.gs_depth_normals(B, S, H, W, vp(depth_acc.data_ptr()), vp(alphas.data_ptr()), vp(K.data_ptr()),
                                        float(min_alpha), vp(normals.data_ptr()),
                                        vp(torch.cuda.current_stream().cuda_stream)), "depth_normals")
    return normals


def normal_loss_hip(depth_acc: Tensor, alphas: Tensor, intrins, prior: Optional[Tensor] = None,
                    guide: Optional[Tensor] = None, prior_weight: float = 1.0, smooth_weight: float = 0.0,
                    edge_beta: float = 0.0, min_alpha: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """gs_normal_loss on GPU tensors: depth_acc, alphas [B,S,H,W], intrins [B,4], prior / guide [B,H,W,3] or None ->
    (loss [B], stats float64 [B,6], normals [B,H,W,3], v_depth_acc [B,S,H,W], v_alphas [B,S,H,W])"""
    _sums.check_hip(depth_acc)
    checked = _check(depth_acc, alphas, intrins, prior, guide, prior_weight, smooth_weight, edge_beta, min_alpha)
    return _launch_loss(*checked[:5], prior_weight, smooth_weight, edge_beta, min_alpha)


def _launch_loss(depth_acc, alphas, K, prior, guide, prior_weight, smooth_weight, edge_beta, min_alpha):
    """normal_loss_hip on what _check returned"""
    depth_acc, alphas = depth_acc.contiguous(), alphas.contiguous()
    prior = None if prior is None else prior.contiguous()
    guide = None if guide is None else guide.contiguous()
    B, _, H, W = (int(s) for s in depth_acc.shape)
    dev = depth_acc.device
    normals = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    vp = ctypes.c_void_p
    loss, stats, v_depth_acc, v_alphas = _sums.launch_loss(
        "normal_loss", "gs_normal_loss_workspace_bytes", depth_acc, alphas, STATS,
        lambda lib, head, outs, tail: lib.gs_normal_loss(
            *head, vp(_device_intrins(K, dev).data_ptr()), vp(prior.data_ptr()) if prior is not None else None,
            vp(guide.data_ptr()) if guide is not None else None, float(prior_weight), float(smooth_weight), float(edge_beta),
            float(min_alpha), *outs, vp(normals.data_ptr()), *tail))
    return loss, stats, normals, v_depth_acc, v_alphas


# --------------------------------------------------------------------------- #
# torch restatement (CPU tensors)
# --------------------------------------------------------------------------- #
def _shift(t: Tensor, dy: int, dx: int) -> Tensor:
    """out[:, v, u] = t[:, v + dy, u + dx], zeros where that is outside; t [B,H,W,...]"""
    out = torch.zeros_like(t)
    H, W = t.shape[1], t.shape[2]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if H - abs(dy) > 0 and W - abs(dx) > 0:
        out[:, yd, xd] = t[:, ys, xs]
    return out


def _cross(a: Tensor, b: Tensor) -> Tensor:
    """a x b on the last axis, two products and one difference per component, each rounded"""
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)


def _geometry(acc4: Tensor, al4: Tensor, K: Tensor, min_alpha: float):
    """the float32 part of csrc/normal_math.h on [B,S,H,W]: -> d, a, has_z [B,H,W], rx [B,1,W], ry [B,H,1], tx, ty
    [B,H,W,3], l2 [B,H,W], normals [B,H,W,3], defined [B,H,W]"""
    B, S, H, W = (int(s) for s in acc4.shape)
    dev = acc4.device
    f32 = dict(dtype=torch.float32, device=dev)
    d, a = _sums.sample_means(acc4, al4)
    has = (a > torch.tensor(float(min_alpha), **f32)) & (d > 0)
    one = torch.ones((), **f32)
    z = torch.where(has, d, one) / torch.where(has, a, one)
    K = K.to(dev)
    half = torch.tensor(0.5, **f32)
    rx = ((torch.arange(W, **f32)[None, None, :] + half) - K[:, 2, None, None]) / K[:, 0, None, None]
    ry = ((torch.arange(H, **f32)[None, :, None] + half) - K[:, 3, None, None]) / K[:, 1, None, None]
    P = torch.stack([rx * z, ry * z, z], dim=-1)
    tx = _shift(P, 0, 1) - _shift(P, 0, -1)
    ty = _shift(P, 1, 0) - _shift(P, -1, 0)
    c = _cross(ty, tx)
    l2 = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
    inner = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
    if H >= 3 and W >= 3:
        inner[:, 1:-1, 1:-1] = True
    hz = has[..., None]
    ok = inner & has & _shift(hz, 0, 1)[..., 0] & _shift(hz, 0, -1)[..., 0] & _shift(hz, 1, 0)[..., 0] & \
        _shift(hz, -1, 0)[..., 0] & (l2 > torch.tensor(MIN_L2, **f32))
    n = torch.where(ok[..., None], c / torch.sqrt(torch.where(ok, l2, one))[..., None], torch.zeros((), **f32))
    defined = (n != 0).any(dim=-1)
    return d, a, has, rx, ry, tx, ty, l2, n, defined


def depth_normals_torch(depth_acc: Tensor, alphas: Tensor, intrins, min_alpha: float = 0.0) -> Tensor:
    """depth_normals as torch ops on the tensors' device (csrc/normal_math.h operation by operation)"""
    acc4, al4, K, _, _, single = _check(depth_acc, alphas, intrins, min_alpha=min_alpha)
    n = _geometry(acc4, al4, K, min_alpha)[8]
    return n[0] if single else n


def _prior_units(prior: Tensor):
    l = (prior[..., 0] * prior[..., 0] + prior[..., 1] * prior[..., 1]) + prior[..., 2] * prior[..., 2]
    has = (l > 0) & (l < float("inf"))
    r = torch.sqrt(torch.where(has, l, torch.ones_like(l)))
    return torch.where(has[..., None], prior / r[..., None], torch.zeros_like(prior)), has


def _pair_weight(guide: Optional[Tensor], like: Tensor, edge_beta: float, dy: int, dx: int) -> Tensor:
    """g between every pixel and its neighbour at (+dy, +dx), float32 [B,H,W] (whatever it is where no neighbour exists)"""
    if guide is None or not edge_beta > 0:
        return torch.ones_like(like)
    diff = (guide - _shift(guide, dy, dx)).abs()
    s = (diff[..., 0] + diff[..., 1]) + diff[..., 2]
    beta = torch.tensor(float(edge_beta), dtype=torch.float32, device=like.device)
    return torch.exp(-(beta * (s / torch.tensor(3.0, dtype=torch.float32, device=like.device))))


def normal_loss_torch(depth_acc: Tensor, alphas: Tensor, intrins, prior: Optional[Tensor] = None,
                      guide: Optional[Tensor] = None, prior_weight: float = 1.0, smooth_weight: float = 0.0,
                      edge_beta: float = 0.0, min_alpha: float = 0.0, return_stats: bool = False,
                      return_normals: bool = False):
    """the operations of csrc/normal_math.h one by one as torch ops on the tensors' device: float32 per pixel, float64 sums
    and gradient chain.  Shapes and results as normal_loss_with_grad"""
    acc4, al4, K, prior, guide, single = _check(depth_acc, alphas, intrins, prior, guide, prior_weight, smooth_weight,
                                                edge_beta, min_alpha)
    B, S, H, W = (int(s) for s in acc4.shape)
    d, a, has, rx, ry, tx, ty, l2, n, defined = _geometry(acc4, al4, K, min_alpha)
    pw = float(torch.tensor(float(prior_weight), dtype=torch.float32))     # the C ABI takes the weights as floats
    sw = float(torch.tensor(float(smooth_weight), dtype=torch.float32))
    n64 = n.double()
    zero = torch.zeros((), dtype=torch.float64, device=acc4.device)

    def tot(t):
        return t.reshape(B, -1).sum(dim=1)
    if prior is not None:
        m, has_m = _prior_units(prior)
        m64 = torch.where((has_m & defined)[..., None], m.double(), zero)
        use = has_m & defined
    else:
        m64, use = torch.zeros_like(n64), torch.zeros_like(defined)
    n_p = tot(use.double())
    s_p = tot(torch.where(use, 1.0 - (n64 * m64).sum(-1), zero))
    # the four neighbours in the header's order: left, right, upper, lower
    pair_sum = torch.zeros_like(n64)
    n_s, s_s, s_g = torch.zeros_like(n_p), torch.zeros_like(n_p), torch.zeros_like(n_p)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        both = defined & _shift(defined[..., None], dy, dx)[..., 0]
        g = torch.where(both, _pair_weight(guide, l2, edge_beta, dy, dx).double(), zero)
        nq = _shift(n64, dy, dx)
        pair_sum = pair_sum + g[..., None] * nq
        if dy + dx > 0:                                        # the pairs a pixel owns: q = p + x, p + y
            n_s = n_s + tot(both.double())
            s_s = s_s + tot(g * torch.where(both, 1.0 - (n64 * nq).sum(-1), zero))
            s_g = s_g + tot(g)
    col = (slice(None), None, None, None)
    kp = torch.where(n_p >= 1, pw / torch.clamp(n_p, min=1.0), zero)
    ks = torch.where(n_s >= 1, sw / torch.clamp(n_s, min=1.0), zero)
    loss = kp * s_p + ks * s_s
    vn = -(kp[col] * m64) - ks[col] * pair_sum
    r = torch.sqrt(torch.where(defined, l2.double(), zero + 1.0))
    vc = (vn - n64 * (n64 * vn).sum(-1, keepdim=True)) / r[..., None]
    vc = torch.where(defined[..., None], vc, zero)
    vty, vtx = _cross(tx.double(), vc), _cross(vc, ty.double())
    vP = _shift(vtx, 0, -1) - _shift(vtx, 0, 1) + _shift(vty, -1, 0) - _shift(vty, 1, 0)
    vz = rx.double() * vP[..., 0] + ry.double() * vP[..., 1] + vP[..., 2]
    d64, a64 = torch.where(has, d.double(), zero + 1.0), torch.where(has, a.double(), zero + 1.0)
    gd = torch.where(has, (vz / a64) / float(S), zero).float()
    ga = torch.where(has, (-(vz * d64) / (a64 * a64)) / float(S), zero).float()
    v_acc = gd[:, None].expand(B, S, H, W).contiguous()
    v_al = ga[:, None].expand(B, S, H, W).contiguous()
    loss = loss.float()
    stats = torch.stack([tot(defined.double()), n_p, s_p, n_s, s_s, s_g], dim=1)
    loss, v_acc, v_al, stats, n = _sums.unbatch((loss, v_acc, v_al, stats, n), single)
    return (loss, v_acc, v_al) + ((stats,) if return_stats else ()) + ((n,) if return_normals else ())


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def depth_normals(depth_acc: Tensor, alphas: Tensor, intrins, min_alpha: float = 0.0) -> Tensor:
    """Normals of the depth z = d / a (module docstring): depth_acc, alphas [S,H,W] -> [H,W,3]; [B,S,H,W] -> [B,H,W,3].
    intrins: fx, fy, cx, cy of the camera the frame was rendered with (4 floats, or [B,4]).  Camera-frame unit vectors
    facing the camera, (0, 0, 0) where there is none; an image with H < 3 or W < 3 has none.  No gradient (normal_loss is
    the differentiable op).  HIP tensors take the kernel, CPU tensors depth_normals_torch."""
    if not isinstance(depth_acc, Tensor):
        raise ValueError("depth_acc must be a tensor")
    if not depth_acc.is_cuda:
        return depth_normals_torch(depth_acc, alphas, intrins, min_alpha)
    acc4, al4, K, _, _, single = _check(depth_acc, alphas, intrins, min_alpha=min_alpha)
    n = depth_normals_hip(acc4, al4, K, min_alpha)
    return n[0] if single else n


def normal_loss_with_grad(depth_acc: Tensor, alphas: Tensor, intrins, prior: Optional[Tensor] = None,
                          guide: Optional[Tensor] = None, prior_weight: float = 1.0, smooth_weight: float = 0.0,
                          edge_beta: float = 0.0, min_alpha: float = 0.0, return_stats: bool = False,
                          return_normals: bool = False):
    """(loss, d loss / d depth_acc, d loss / d alphas[, stats][, normals]) in one call — the form for the one-call training
    route (SplatfactoDeblurModel.render_and_backward grad_depth_sums).  depth_acc, alphas [S,H,W] with prior / guide
    [H,W,3] or None -> loss a scalar; [B,S,H,W] with [B,H,W,3] -> loss [B], each frame's gradients those of its own loss.
    prior: a zero or non-finite vector means no value; it is normalised here.  guide: the image whose edges relax the
    smoothness term (a constant; used with edge_beta > 0).  stats: float64 [(B,) 6] = normals, Np, Σ(1 − n·m), Ns,
    Σ g (1 − n_p·n_q), Σ g.  HIP tensors take the kernels, CPU tensors normal_loss_torch.  ValueError for a wrong shape,
    dtype, device or weight.  Nothing is recorded for autograd (normal_loss is the autograd form)."""
    if not isinstance(depth_acc, Tensor):
        raise ValueError("depth_acc must be a tensor")
    if not depth_acc.is_cuda:
        return normal_loss_torch(depth_acc, alphas, intrins, prior, guide, prior_weight, smooth_weight, edge_beta,
                                 min_alpha, return_stats, return_normals)
    acc4, al4, K, pr4, gd4, single = _check(depth_acc, alphas, intrins, prior, guide, prior_weight, smooth_weight,
                                            edge_beta, min_alpha)
    loss, stats, n, v_acc, v_al = _sums.unbatch(
        _launch_loss(acc4, al4, K, pr4, gd4, prior_weight, smooth_weight, edge_beta, min_alpha), single)
    return (loss, v_acc, v_al) + ((stats,) if return_stats else ()) + ((n,) if return_normals else ())


def normal_loss(depth_acc: Tensor, alphas: Tensor, intrins, prior: Optional[Tensor] = None, guide: Optional[Tensor] = None,
                prior_weight: float = 1.0, smooth_weight: float = 0.0, edge_beta: float = 0.0,
                min_alpha: float = 0.0) -> Tensor:
    """The normal loss (module docstring) of depth_acc, alphas [S,H,W]: a scalar; or of [B,S,H,W]: [B], one loss per frame.
    Differentiable in depth_acc and alphas (an autograd Function; intrins, prior and guide are constants).  Arguments as
    normal_loss_with_grad."""
    return _sums.SumsLoss.apply(normal_loss_with_grad, depth_acc, alphas, intrins, prior, guide, float(prior_weight),
                                float(smooth_weight), float(edge_beta), float(min_alpha))
