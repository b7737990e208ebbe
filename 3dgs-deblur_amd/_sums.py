"""What the losses on the compositor's raw per-sample sums share (depthprior.py, normals.py): the limits, the checks of
depth_acc and alphas, the sample means of the torch restatements, the outputs and workspace around the C call, and the
autograd form.  Device counterpart: csrc/sums_loss.h."""
from __future__ import annotations

import ctypes
from typing import Callable, Tuple

import torch
from torch import Tensor

MAX_PLANES = 256                     # B * S
MAX_ELEMS = 1 << 30                  # B * S * H * W stays below it


def check_sums(who: str, depth_acc, alphas, **images) -> Tuple[Tensor, Tensor, bool]:
    """-> (depth_acc [B,S,H,W], alphas, single), detached; ValueError for anything else.  who: the subject of the limits'
    message ("depth_prior_loss supports"); images: further tensors (or None) that must be float32 on depth_acc's device"""
    if not isinstance(depth_acc, Tensor) or depth_acc.dtype != torch.float32:
        raise ValueError("depth_acc must be a float32 tensor")
    for name, t in (("alphas", alphas), *images.items()):
        if t is None and name != "alphas":
            continue
        if not isinstance(t, Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if t.device != depth_acc.device:
            raise ValueError(f"{name} is on {t.device}, depth_acc on {depth_acc.device}")
    if depth_acc.dim() not in (3, 4):
        raise ValueError(f"depth_acc must be [S,H,W] or [B,S,H,W], got {tuple(depth_acc.shape)}")
    if alphas.shape != depth_acc.shape:
        raise ValueError(f"alphas must have depth_acc's shape {tuple(depth_acc.shape)}, got {tuple(alphas.shape)}")
    single = depth_acc.dim() == 3
    depth_acc, alphas = depth_acc.detach(), alphas.detach()
    if single:
        depth_acc, alphas = depth_acc[None], alphas[None]
    B, S, H, W = (int(s) for s in depth_acc.shape)
    if S < 1 or H < 1 or W < 1:
        raise ValueError(f"depth_acc needs at least one sample and one pixel, got {tuple(depth_acc.shape)}")
    if B * S > MAX_PLANES or max(B, 1) * S * H * W >= MAX_ELEMS:
        raise ValueError(f"{who} B * S <= {MAX_PLANES} and B * S * H * W < 2^30, got B={B}, S={S}, H={H}, W={W}")
    return depth_acc, alphas, single


def check_hip(depth_acc) -> None:
    """the *_hip functions take [B,S,H,W] on the GPU only"""
    if not isinstance(depth_acc, Tensor) or not depth_acc.is_cuda:
        raise ValueError("depth_acc must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    if depth_acc.dim() != 4:
        raise ValueError(f"depth_acc must be [B,S,H,W], got {tuple(depth_acc.shape)}")


def sample_means(acc4: Tensor, al4: Tensor) -> Tuple[Tensor, Tensor]:
    """d, a [B,H,W]: the float32 means over S with the samples added in order (not .mean), as sample_mean of
    csrc/depthprior_math.h"""
    S = int(acc4.shape[1])
    d, a = acc4[:, 0], al4[:, 0]
    for s in range(1, S):
        d, a = d + acc4[:, s], a + al4[:, s]
    Sf = torch.tensor(float(S), dtype=torch.float32, device=acc4.device)
    return d / Sf, a / Sf


def unbatch(results: tuple, single: bool) -> tuple:
    """the results of a [1,S,H,W] call that was given [S,H,W]"""
    return tuple(t[0] for t in results) if single else results


def launch_loss(what: str, workspace_bytes: str, depth_acc: Tensor, alphas: Tensor, n_stats: int, call: Callable):
    """The C call of the loss `what` on contiguous GPU sums [B,S,H,W]: allocates loss [B], stats float64 [B,n_stats],
    v_depth_acc, v_alphas and the workspace the entry point named workspace_bytes asks for, runs call(lib, head, outs, tail)
    — head = B, S, H, W and the two inputs, outs = loss, stats, tail = v_depth_acc, v_alphas, ws, ws_bytes, stream, as the
    entry points order them — and checks its status.  -> (loss, stats, v_depth_acc, v_alphas)"""
    from . import _lib
    B, S, H, W = (int(s) for s in depth_acc.shape)
    dev = depth_acc.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, n_stats, dtype=torch.float64, device=dev)
    v_depth_acc, v_alphas = torch.empty_like(depth_acc), torch.empty_like(alphas)
    if B == 0:
        return loss, stats, v_depth_acc, v_alphas
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(dev):
        ws_bytes = int(getattr(lib, workspace_bytes)(B, S, H, W))
        if ws_bytes < 0:
            raise _lib.HipLibraryError(f"{what}: unsupported shape B={B}, S={S}, H={H}, W={W}")
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
        _lib.check(call(lib, (B, S, H, W, vp(depth_acc.data_ptr()), vp(alphas.data_ptr())),
                        (vp(loss.data_ptr()), vp(stats.data_ptr())),
                        (vp(v_depth_acc.data_ptr()), vp(v_alphas.data_ptr()), vp(ws.data_ptr()), ws_bytes,
                         vp(torch.cuda.current_stream().cuda_stream))), what)
    return loss, stats, v_depth_acc, v_alphas


class SumsLoss(torch.autograd.Function):
    """apply(with_grad, depth_acc, alphas, *constants): the gradients come out of the forward call
    with_grad(depth_acc, alphas, *constants) -> (loss, v_depth_acc, v_alphas); backward scales them by the incoming gradient"""

    @staticmethod
    def forward(ctx, with_grad, depth_acc, alphas, *constants):
        loss, v_acc, v_al = with_grad(depth_acc, alphas, *constants)
        ctx.save_for_backward(v_acc, v_al)
        ctx.constants = len(constants)
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        v_acc, v_al = ctx.saved_tensors
        scale = v_loss if v_loss.dim() == 0 else v_loss.reshape(-1, 1, 1, 1)
        return (None, v_acc * scale if ctx.needs_input_grad[1] else None, v_al * scale if ctx.needs_input_grad[2] else None,
                *([None] * ctx.constants))
