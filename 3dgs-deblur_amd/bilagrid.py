"""Bilateral-grid colour correction (Chen et al. 2007; as a per-image learned correction: gsplat's ``lib_bilagrid`` /
``fused-bilagrid``, nerfstudio splatfacto's ``use_bilateral_grid``) between the compositor and the loss.

Handheld phone video drifts in exposure and white balance from frame to frame; a Gaussian model trained on it bakes the
drift in as view-dependent floaters.  Each training image owns a small 3-D lattice of affine colour transforms
``grids[i]`` ``[12, L, GH, GW]``; a pixel samples it at (x, y, luma of the render) and the interpolated 3x4 transform is
applied to the render before the loss.  The lattices are learned with the scene and kept smooth by a total-variation
penalty.  Evaluation renders are never corrected.

Neither gsplat nor nerfstudio is part of the reference tree: the formulas are recollected (csrc/bilagrid_math.h states
them).  On GPU tensors the HIP kernels of csrc/bilagrid.hip are the only route (``gs_bilagrid_slice_fwd`` /
``gs_bilagrid_slice_bwd`` / ``gs_bilagrid_tv_fwd_bwd``: no float atomics, every sum in a fixed order); the torch
restatements below serve CPU tensors (the host-logic tests) and the ``GSD_TORCH_TRAIN`` A/B switch, as in mcmc.py.  They
are written from the same formulas and do not call ``grid_sample``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor
from torch.autograd import Function

CHANNELS = 12                        # csrc/bilagrid_math.h kChannels: row-major 3x4 [A | b]
DEFAULT_SHAPE = (16, 16, 8)          # (GW, GH, L)
LUMA = (0.299, 0.587, 0.114)


def identity_grids(G: int, shape: Sequence[int] = DEFAULT_SHAPE, device=None) -> Tensor:
    """[G, 12, L, GH, GW] float32 with A = I, b = 0 at every vertex; shape = (GW, GH, L), every axis >= 2"""
    GW, GH, L = (int(s) for s in shape)
    if min(GW, GH, L) < 2 or G < 0:
        raise ValueError(f"grid shape (GW, GH, L) = {(GW, GH, L)}: every axis must be >= 2")
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32, device=device)
    return eye.reshape(1, CHANNELS, 1, 1, 1).repeat(G, 1, L, GH, GW)


def _use_hip(t: Tensor) -> bool:
    from .train_step import TORCH_TRAIN
    return t.is_cuda and not TORCH_TRAIN


def _f32c(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _check_grids(grids: Tensor) -> Tuple[int, int, int, int]:
    if grids.dim() != 5 or grids.shape[1] != CHANNELS or min(grids.shape[2:]) < 2:
        raise ValueError(f"grids must be [G, 12, L, GH, GW] with every lattice axis >= 2, got {tuple(grids.shape)}")
    G, _, L, GH, GW = (int(s) for s in grids.shape)
    return G, GW, GH, L


_IDX_CACHE = {}


def _index_tensor(grid_idx, B: int, G: int, device) -> Tensor:
    """grid_idx (int, sequence of ints or tensor [B]) -> contiguous int32 [B] on `device`.  Host integers are range-checked
    here and uploaded once per distinct tuple (a fresh upload is a pageable copy, i.e. a stream synchronisation per
    step); a device tensor is the caller's responsibility — the kernels pass an image whose index is outside [0, G)
    through unchanged"""
    if isinstance(grid_idx, Tensor):
        if grid_idx.numel() != B:
            raise ValueError(f"grid_idx must hold {B} indices, got {grid_idx.numel()}")
        if not grid_idx.is_cuda and grid_idx.device != torch.device(device):
            grid_idx = tuple(int(i) for i in grid_idx.reshape(-1).tolist())
        else:
            return grid_idx.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    idx = (int(grid_idx),) if isinstance(grid_idx, int) else tuple(int(i) for i in grid_idx)
    if len(idx) != B:
        raise ValueError(f"grid_idx must hold {B} indices, got {len(idx)}")
    if any(i < 0 or i >= G for i in idx):
        raise ValueError(f"grid_idx {idx} outside [0, {G})")
    key = (idx, str(device))
    t = _IDX_CACHE.get(key)
    if t is None:
        if len(_IDX_CACHE) > 4096:
            _IDX_CACHE.clear()
        t = _IDX_CACHE[key] = torch.tensor(idx, dtype=torch.int32, device=device)
    return t


def _batched(rgb: Tensor) -> Tuple[Tensor, bool]:
    if rgb.dim() == 3 and rgb.shape[-1] == 3:
        return rgb[None], True
    if rgb.dim() == 4 and rgb.shape[-1] == 3:
        return rgb, False
    raise ValueError(f"rgb must be [H,W,3] or [B,H,W,3], got {tuple(rgb.shape)}")


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
def slice_fwd_hip(grids: Tensor, rgb: Tensor, idx: Tensor) -> Tensor:
    """gs_bilagrid_slice_fwd: grids [G,12,L,GH,GW], rgb [B,H,W,3], idx int32 [B] (device) -> corrected [B,H,W,3]"""
    from . import _lib
    grids, rgb = _f32c(grids, "grids"), _f32c(rgb, "rgb")
    G, GW, GH, L = _check_grids(grids)
    B, H, W = (int(s) for s in rgb.shape[:3])
    out = torch.empty_like(rgb)
    if B == 0 or G == 0 or H == 0 or W == 0:
        return out.copy_(rgb)
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(rgb.device):
        _lib.check(lib.gs_bilagrid_slice_fwd(B, H, W, G, GW, GH, L, vp(grids.data_ptr()), vp(idx.data_ptr()),
                                             vp(rgb.data_ptr()), vp(out.data_ptr()),
                                             vp(torch.cuda.current_stream().cuda_stream)), "bilagrid_slice_fwd")
    return out


def slice_bwd_hip(grids: Tensor, rgb: Tensor, idx: Tensor, v_out: Tensor) -> Tuple[Tensor, Tensor]:
    """gs_bilagrid_slice_bwd -> (v_rgb [B,H,W,3], v_grids [G,12,L,GH,GW]); bit-identical from run to run"""
    from . import _lib
    grids, rgb, v_out = _f32c(grids, "grids"), _f32c(rgb, "rgb"), _f32c(v_out, "v_out")
    G, GW, GH, L = _check_grids(grids)
    B, H, W = (int(s) for s in rgb.shape[:3])
    if v_out.shape != rgb.shape:
        raise ValueError("v_out must have rgb's shape")
    if B == 0 or G == 0 or H == 0 or W == 0:
        return v_out.clone(), torch.zeros_like(grids)
    v_rgb, v_grids = torch.empty_like(rgb), torch.empty_like(grids)
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(rgb.device):
        ws_bytes = lib.gs_bilagrid_slice_bwd_workspace_bytes(B, H, W, G, GW, GH, L)
        if ws_bytes < 0:
            raise _lib.HipLibraryError("bilagrid_slice_bwd: no tile of this frame fits its lattice footprint in LDS")
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=rgb.device)
        _lib.check(lib.gs_bilagrid_slice_bwd(B, H, W, G, GW, GH, L, vp(grids.data_ptr()), vp(idx.data_ptr()),
                                             vp(rgb.data_ptr()), vp(v_out.data_ptr()), vp(v_rgb.data_ptr()),
                                             vp(v_grids.data_ptr()), vp(ws.data_ptr()), int(ws_bytes),
                                             vp(torch.cuda.current_stream().cuda_stream)), "bilagrid_slice_bwd")
    return v_rgb, v_grids


def tv_fwd_bwd_hip(grids: Tensor, weight: float, v_grids: Optional[Tensor] = None) -> Tensor:
    """gs_bilagrid_tv_fwd_bwd: -> weight * tv(grids) as a 0-dim device tensor; v_grids (optional, grids' shape) +=
    weight * d tv / d grids.  One call, nothing is read back."""
    from . import _lib
    grids = _f32c(grids, "grids")
    G, GW, GH, L = _check_grids(grids)
    out = torch.zeros(1, dtype=torch.float32, device=grids.device)
    if G == 0:
        return out[0]
    if v_grids is not None:
        if v_grids.shape != grids.shape or not v_grids.is_cuda or v_grids.dtype != torch.float32 \
                or not v_grids.is_contiguous():
            raise ValueError("v_grids must be a contiguous float32 GPU tensor of grids' shape")
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(grids.device):
        ws_bytes = int(lib.gs_bilagrid_tv_workspace_bytes(G, GW, GH, L))
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=grids.device)
        _lib.check(lib.gs_bilagrid_tv_fwd_bwd(G, GW, GH, L, vp(grids.data_ptr()), float(weight), vp(out.data_ptr()),
                                              vp(v_grids.data_ptr() if v_grids is not None else None),
                                              vp(ws.data_ptr()), ws_bytes,
                                              vp(torch.cuda.current_stream().cuda_stream)), "bilagrid_tv_fwd_bwd")
    return out[0]


# --------------------------------------------------------------------------- #
# torch restatements (CPU tensors, A/B)
# --------------------------------------------------------------------------- #
def _axis(c: Tensor, n: int):
    """coordinate in [0,1] (clamped) on an axis of n vertices -> (lower vertex int64, fraction); differentiable in c
    where it was not clamped"""
    p = c.clamp(0.0, 1.0) * (n - 1)
    i0 = p.detach().floor().clamp(0, n - 2)
    return i0.long(), p - i0


def slice_torch(grids: Tensor, rgb: Tensor, idx: Tensor) -> Tensor:
    """the slice as torch ops, from csrc/bilagrid_math.h's formulas: eight gathers and their trilinear weights.
    Differentiable in grids and rgb (through A and through the guide).  grids [G,12,L,GH,GW], rgb [B,H,W,3], idx [B]."""
    G, GW, GH, L = _check_grids(grids)
    B, H, W, _ = rgb.shape
    dt, dev = rgb.dtype, rgb.device
    x0, fx = _axis((torch.arange(W, device=dev, dtype=dt) + 0.5) / W, GW)
    y0, fy = _axis((torch.arange(H, device=dev, dtype=dt) + 0.5) / H, GH)
    luma = rgb[..., 0] * LUMA[0] + rgb[..., 1] * LUMA[1] + rgb[..., 2] * LUMA[2]
    z0, fz = _axis(luma, L)                                                   # [B,H,W]
    flat = grids.to(dt)[idx.long()].permute(0, 2, 3, 4, 1).reshape(B, L * GH * GW, CHANNELS)
    x0, fx = x0.reshape(1, 1, W), fx.reshape(1, 1, W)
    y0, fy = y0.reshape(1, H, 1), fy.reshape(1, H, 1)
    A = None
    for dz in (0, 1):
        wz = fz if dz else 1.0 - fz
        for dy in (0, 1):
            wy = fy if dy else 1.0 - fy
            for dx in (0, 1):
                wx = fx if dx else 1.0 - fx
                v = ((z0 + dz) * GH + (y0 + dy)) * GW + (x0 + dx)             # [B,H,W]
                vals = flat.gather(1, v.reshape(B, H * W, 1).expand(B, H * W, CHANNELS)).reshape(B, H, W, CHANNELS)
                term = (wz * wy * wx)[..., None] * vals
                A = term if A is None else A + term
    M = A.reshape(B, H, W, 3, 4)
    return (M[..., :3] * rgb[..., None, :]).sum(-1) + M[..., 3]


def tv_torch(grids: Tensor) -> Tensor:
    """2 * (mean squared forward difference along x + along y + along z), over all images, channels and positions"""
    dx = grids[..., :, :, 1:] - grids[..., :, :, :-1]
    dy = grids[..., :, 1:, :] - grids[..., :, :-1, :]
    dz = grids[..., 1:, :, :] - grids[..., :-1, :, :]
    return 2.0 * ((dx * dx).mean() + (dy * dy).mean() + (dz * dz).mean())


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def slice_fwd(grids: Tensor, rgb: Tensor, grid_idx) -> Tensor:
    """the forward half (no autograd graph): corrected image(s), rgb's shape"""
    rgb4, single = _batched(rgb)
    G = _check_grids(grids)[0]
    idx = _index_tensor(grid_idx, rgb4.shape[0], G, rgb4.device)
    with torch.no_grad():
        out = slice_fwd_hip(grids.detach(), rgb4.detach(), idx) if _use_hip(rgb4) else slice_torch(grids, rgb4, idx)
    return out[0] if single else out


def slice_bwd(grids: Tensor, rgb: Tensor, grid_idx, v_out: Tensor) -> Tuple[Tensor, Tensor]:
    """the backward half: (d loss / d rgb in rgb's shape, d loss / d grids [G,12,L,GH,GW]) from d loss / d corrected"""
    rgb4, single = _batched(rgb)
    G = _check_grids(grids)[0]
    idx = _index_tensor(grid_idx, rgb4.shape[0], G, rgb4.device)
    v4 = v_out[None] if single else v_out
    if _use_hip(rgb4):
        v_rgb, v_grids = slice_bwd_hip(grids.detach(), rgb4.detach(), idx, v4.detach())
    else:
        with torch.enable_grad():
            g_, r_ = grids.detach().requires_grad_(True), rgb4.detach().requires_grad_(True)
            v_rgb, v_grids = torch.autograd.grad(slice_torch(g_, r_, idx), (r_, g_), v4.detach().to(r_.dtype))
        v_grids = v_grids.to(grids.dtype)
    return (v_rgb[0] if single else v_rgb), v_grids


class _Slice(Function):
    @staticmethod
    def forward(ctx, grids, rgb4, idx):
        ctx.save_for_backward(grids, rgb4, idx)
        return slice_fwd_hip(grids, rgb4, idx)

    @staticmethod
    def backward(ctx, v_out):
        grids, rgb4, idx = ctx.saved_tensors
        v_rgb, v_grids = slice_bwd_hip(grids, rgb4, idx, v_out)
        return v_grids, v_rgb, None


def slice(grids: Tensor, rgb: Tensor, grid_idx: Union[int, Sequence[int], Tensor]) -> Tensor:     # noqa: A001
    """Apply each image's bilateral grid: rgb [H,W,3] with an int index, or [B,H,W,3] with B indices (host integers or an
    int tensor [B]; two images may share a grid) -> corrected image(s) of rgb's shape.  Differentiable in grids and rgb.
    HIP tensors take the kernels (one autograd node), CPU tensors the torch restatement."""
    rgb4, single = _batched(rgb)
    G = _check_grids(grids)[0]
    idx = _index_tensor(grid_idx, rgb4.shape[0], G, rgb4.device)
    if grids.device != rgb4.device:
        raise ValueError("grids and rgb must live on the same device")
    out = _Slice.apply(grids, rgb4, idx) if _use_hip(rgb4) else slice_torch(grids, rgb4, idx)
    return out[0] if single else out


class _TV(Function):
    @staticmethod
    def forward(ctx, grids, weight):
        v = torch.zeros_like(grids, memory_format=torch.contiguous_format)
        loss = tv_fwd_bwd_hip(grids, weight, v)
        ctx.save_for_backward(v)
        return loss.clone()

    @staticmethod
    def backward(ctx, v_loss):
        (v,) = ctx.saved_tensors
        return v * v_loss, None


def tv_loss(grids: Tensor, weight: float = 1.0) -> Tensor:
    """weight * tv(grids): tv = 2 (m_x + m_y + m_z), m_a the mean squared forward difference along lattice axis a over
    all images, channels and positions.  On HIP tensors value and gradient come from ONE kernel call."""
    _check_grids(grids)
    if _use_hip(grids):
        return _TV.apply(grids, float(weight))
    return float(weight) * tv_torch(grids)
