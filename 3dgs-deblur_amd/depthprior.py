"""Scale- and shift-invariant depth-prior loss: a monocular depth prior (MiDaS, Depth Anything: known only up to an
unknown scale and shift, usually as inverse depth) against the rendered depth.

``kind="pearson"`` is the correlation loss of the depth-regularised 3DGS methods for sparse or casual captures (FSGS,
SparseGS; recollected, none of them is part of the reference tree): ``weight * (1 - Pearson(x, prior))`` over the valid
pixels, which no scale and no shift of the prior changes.  ``kind="l1"`` is ``weight * mean |x - prior|`` over the same
pixels, for a prior in the units of x.  It is NOT ``train_step.depth_loss``: that one also counts the pixels the render
does not cover, against the far value ``expected_depth`` fills them with; here an uncovered pixel is invalid.

The op starts from the compositor's raw per-sample sums (csrc/depthprior_math.h states every operation): depth_acc and
alphas [S,H,W], ``d`` and ``a`` their sample means added in order, a pixel valid where ``prior > 0 and a > min_alpha``
(and ``d > 0`` in disparity space), ``x = d / a`` for ``space="depth"``, ``x = a / d`` for ``space="disparity"``.
Per-pixel values are float32 with every operation rounded, the sums and the gradient chain float64.  A frame with fewer
than two valid pixels, a constant render or a constant prior has no correlation: loss 0 and exact zero gradients.

On HIP tensors the kernels of csrc/depthprior.hip are the only route (``gs_depth_prior_loss``: two launches, no atomics,
nothing read back, bit-identical from run to run and independent of the rest of the batch); CPU tensors take
``depth_prior_loss_torch``, the same operations as torch ops."""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch
from torch import Tensor

from . import _sums
from ._sums import MAX_ELEMS, MAX_PLANES  # noqa: F401  (the limits of every loss on the sums)

KINDS = ("pearson", "l1")            # csrc/depthprior_math.h kPearson, kL1
SPACES = ("depth", "disparity")      # kDepth, kDisparity
STATS = 8                            # kStats: n, sum x, sum y, sum xx, sum yy, sum xy, sum |x - y|, rho
DEGENERATE_TOL = 1e-12               # kDegenerateTol


def _check(depth_acc, alphas, prior, kind, space, weight, min_alpha) -> Tuple[Tensor, Tensor, Tensor, bool]:
    """-> (depth_acc [B,S,H,W], alphas, prior [B,H,W], single), detached; ValueError for anything else"""
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r} (one of {KINDS})")
    if space not in SPACES:
        raise ValueError(f"unknown space {space!r} (one of {SPACES})")
    if not isinstance(prior, Tensor):
        raise ValueError("prior must be a float32 tensor")
    depth_acc, alphas, single = _sums.check_sums("depth_prior_loss supports", depth_acc, alphas, prior=prior)
    B, _, H, W = (int(s) for s in depth_acc.shape)
    want = (H, W) if single else (B, H, W)
    if tuple(prior.shape) != want:
        raise ValueError(f"prior must be {list(want)}, got {tuple(prior.shape)}")
    if not float(min_alpha) >= 0.0:
        raise ValueError(f"min_alpha must be >= 0, got {min_alpha}")
    if not float(weight) == float(weight):
        raise ValueError("weight must be a number")
    prior = prior.detach()
    return depth_acc, alphas, prior[None] if single else prior, single


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
def depth_prior_loss_hip(depth_acc: Tensor, alphas: Tensor, prior: Tensor, kind: str = "pearson", space: str = "depth",
                         weight: float = 1.0, min_alpha: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """gs_depth_prior_loss on GPU tensors: depth_acc, alphas [B,S,H,W], prior [B,H,W] -> (loss [B], stats float64 [B,8],
    v_depth_acc [B,S,H,W], v_alphas [B,S,H,W])"""
    _sums.check_hip(depth_acc)
    return _launch(*_check(depth_acc, alphas, prior, kind, space, weight, min_alpha)[:3], kind, space, weight, min_alpha)


def _launch(depth_acc, alphas, prior, kind, space, weight, min_alpha):
    """depth_prior_loss_hip on what _check returned"""
    depth_acc, alphas, prior = depth_acc.contiguous(), alphas.contiguous(), prior.contiguous()
    vp = ctypes.c_void_p
    return _sums.launch_loss("depth_prior_loss", "gs_depth_prior_workspace_bytes", depth_acc, alphas, STATS,
                             lambda lib, head, outs, tail: lib.gs_depth_prior_loss(
                                 *head, vp(prior.data_ptr()), KINDS.index(kind), SPACES.index(space), float(min_alpha),
                                 float(weight), *outs, *tail))


# --------------------------------------------------------------------------- #
# torch restatement (CPU tensors)
# --------------------------------------------------------------------------- #
def depth_prior_loss_torch(depth_acc: Tensor, alphas: Tensor, prior: Tensor, kind: str = "pearson", space: str = "depth",
                           weight: float = 1.0, min_alpha: float = 0.0, return_stats: bool = False):
    """the operations of csrc/depthprior_math.h one by one as torch ops on the tensors' device: float32 per pixel (the
    samples added in order, not .mean), float64 sums and gradient chain.  Shapes and results as
    depth_prior_loss_with_grad; return_stats: also the float64 [(B,) 8] sums"""
    acc4, al4, pr3, single = _check(depth_acc, alphas, prior, kind, space, weight, min_alpha)
    B, S, H, W = (int(s) for s in acc4.shape)
    dev = acc4.device
    f32 = dict(dtype=torch.float32, device=dev)
    d, a = _sums.sample_means(acc4, al4)
    valid = (pr3 > 0) & (a > torch.tensor(float(min_alpha), **f32))
    one = torch.ones((), **f32)
    if space == "disparity":
        valid = valid & (d > 0)
        xf = torch.where(valid, a, one) / torch.where(valid, d, one)
    else:
        xf = torch.where(valid, d, one) / torch.where(valid, a, one)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    x = torch.where(valid, xf.double(), zero)
    y = torch.where(valid, pr3.double(), zero)
    w = float(torch.tensor(float(weight), dtype=torch.float32))     # the C ABI takes the weight as a float

    def tot(t):
        return t.reshape(B, -1).sum(dim=1)
    n, sx, sy, sxx, syy, sxy = tot(valid.double()), tot(x), tot(y), tot(x * x), tot(y * y), tot(x * y)
    sabs = tot((x - y).abs()) if kind == "l1" else torch.zeros_like(n)
    rho = torch.zeros_like(n)
    col = (slice(None), None, None)
    if kind == "l1":
        ok = n >= 1
        loss = w * sabs / torch.clamp(n, min=1.0)
        g = torch.sign(x - y) * (w / torch.clamp(n, min=1.0))[col]
    else:
        vx, vy = n * sxx - sx * sx, n * syy - sy * sy
        ok = (n >= 2) & (vx > DEGENERATE_TOL * n * sxx) & (vy > DEGENERATE_TOL * n * syy)
        root = torch.sqrt(torch.where(ok, vx * vy, torch.ones_like(vx)))
        rho = torch.where(ok, (n * sxy - sx * sy) / root, zero)
        loss = torch.where(ok, w * (1.0 - rho), zero)
        safe_vx = torch.where(ok, vx, torch.ones_like(vx))
        g = -w * ((n[col] * y - sy[col]) / root[col] - rho[col] * (n[col] * x - sx[col]) / safe_vx[col])
    live = valid & ok[col]
    d64, a64 = torch.where(live, d.double(), one.double()), torch.where(live, a.double(), one.double())
    if space == "disparity":
        ga, gd = g / d64, -(g * a64) / (d64 * d64)
    else:
        gd, ga = g / a64, -(g * d64) / (a64 * a64)
    gd = torch.where(live, gd / float(S), zero).float()
    ga = torch.where(live, ga / float(S), zero).float()
    v_acc = gd[:, None].expand(B, S, H, W).contiguous()
    v_al = ga[:, None].expand(B, S, H, W).contiguous()
    loss = loss.float()
    stats = torch.stack([n, sx, sy, sxx, syy, sxy, sabs, rho], dim=1)
    loss, v_acc, v_al, stats = _sums.unbatch((loss, v_acc, v_al, stats), single)
    return (loss, v_acc, v_al, stats) if return_stats else (loss, v_acc, v_al)


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def depth_prior_loss_with_grad(depth_acc: Tensor, alphas: Tensor, prior: Tensor, kind: str = "pearson",
                               space: str = "depth", weight: float = 1.0, min_alpha: float = 0.0, return_stats: bool = False):
    """(loss, d loss / d depth_acc, d loss / d alphas) in one call — the form for the one-call training route
    (SplatfactoDeblurModel.render_and_backward grad_depth_sums).  depth_acc, alphas [S,H,W] with prior [H,W] -> loss a
    scalar; [B,S,H,W] with prior [B,H,W] -> loss [B], each frame's gradients those of its own loss.  All float32 on one
    device; prior 0 (or less): no value.  return_stats: also the float64 [(B,) 8] sums n, Σx, Σy, Σx², Σy², Σxy, Σ|x−y|, ρ.
    HIP tensors take the kernels, CPU tensors depth_prior_loss_torch.  ValueError for a wrong shape, dtype, device, kind
    or space.  Nothing is recorded for autograd: the inputs are detached (depth_prior_loss is the autograd form)."""
    if not isinstance(depth_acc, Tensor):
        raise ValueError("depth_acc must be a tensor")
    if not depth_acc.is_cuda:
        return depth_prior_loss_torch(depth_acc, alphas, prior, kind, space, weight, min_alpha, return_stats)
    acc4, al4, pr3, single = _check(depth_acc, alphas, prior, kind, space, weight, min_alpha)
    loss, stats, v_acc, v_al = _sums.unbatch(_launch(acc4, al4, pr3, kind, space, weight, min_alpha), single)
    return (loss, v_acc, v_al, stats) if return_stats else (loss, v_acc, v_al)


def depth_prior_loss(depth_acc: Tensor, alphas: Tensor, prior: Tensor, kind: str = "pearson", space: str = "depth",
                     weight: float = 1.0, min_alpha: float = 0.0) -> Tensor:
    """The depth-prior loss (module docstring) of depth_acc, alphas [S,H,W] against prior [H,W]: a scalar; or of
    [B,S,H,W] against [B,H,W]: [B], one loss per frame.  Differentiable in depth_acc and alphas (an autograd Function;
    prior is a constant).  kind "pearson" (1 - correlation; invariant to the prior's scale and shift) or "l1"; space
    "depth" (x = d / a) or "disparity" (x = a / d, for a prior given as inverse depth); min_alpha: pixels whose mean alpha
    is not above it are left out.  With a rendered depth map instead of the sums pass depth_acc = depth * m, alphas = m
    for m = (accumulation > 0) as float, one sample: x is then the depth itself."""
    return _sums.SumsLoss.apply(depth_prior_loss_with_grad, depth_acc, alphas, prior, kind, space, float(weight),
                                float(min_alpha))
