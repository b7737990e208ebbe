"""Colour-corrected evaluation metrics (mip-NeRF 360's ``color_correct``; gsplat's ``lib_bilagrid.color_correct``,
nerfstudio splatfacto's ``color_corrected_metrics``): before PSNR / SSIM are taken, the rendered image is fitted to the
ground truth by a per-channel quadratic colour warp, so that a per-frame exposure or white-balance offset of an
evaluation frame — which the bilateral grid, the learnable exposure and the learnable background absorb during training
but no evaluation render corrects — does not pass for a reconstruction error.

None of the upstream projects is part of the reference tree: the algorithm is recollected, csrc/colorcorrect_math.h
states it.  ``num_iters`` times: per output channel c, the weights w_c of the ten features (rr, rg, rb, gg, gb, bb, r, g,
b, 1) of the current image x that minimise the squared error to ref[c] over the pixels whose img[c] (the ORIGINAL
image), x[c] and ref[c] all lie in [eps, 1 - eps]; then x <- clip(a . w, 0, 1) for every pixel.  The sums and the solve
are float64 normal equations; x is stored as float32 between iterations and the three range tests are float32 compares
of the stored values against float32(eps) and float32(1 - eps).

Degenerate rule (departs from upstream, whose lstsq returns a minimum-norm or all-zero warp): a channel with fewer than
10 unmasked pixels, or whose normal matrix is numerically rank-deficient (a Cholesky pivot of the Jacobi-scaled matrix
not above 1e-10), keeps the IDENTITY warp for that iteration.  A black or constant render therefore stays as it is
instead of turning to zero.

On HIP tensors the kernels of csrc/colorcorrect.hip are the only route (``gs_color_correct``: every iteration in one
call, no read-back, no float atomics, bit-identical from run to run and independent of the rest of the batch); CPU
tensors take ``color_correct_torch``, the same rules as torch ops.  The fit is an evaluation tool and carries no gradient.
"""
from __future__ import annotations

import ctypes
from typing import Tuple, Union

import torch
from torch import Tensor

FEATURES = 10                        # csrc/colorcorrect_math.h kFeatures
MIN_COUNT = 10                       # kMinCount
PIVOT_TOL = 1e-10                    # kPivotTol
DEFAULT_EPS = 0.5 / 255


def _batched(img: Tensor, ref: Tensor) -> Tuple[Tensor, Tensor, bool]:
    if img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"img must be [H,W,3] or [B,H,W,3], got {tuple(img.shape)}")
    if ref.shape != img.shape:
        raise ValueError(f"ref must have img's shape {tuple(img.shape)}, got {tuple(ref.shape)}")
    if img.dtype != torch.float32 or ref.dtype != torch.float32:
        raise ValueError(f"img and ref must be float32, got {img.dtype} and {ref.dtype}")
    if img.device != ref.device:
        raise ValueError("img and ref must live on the same device")
    single = img.dim() == 3
    img, ref = img.detach(), ref.detach()
    return (img[None], ref[None], True) if single else (img, ref, False)


def identity_warps(B: int, num_iters: int, device=None) -> Tensor:
    """[B, num_iters, 3, 10] float64: 1 on each channel's own linear feature"""
    w = torch.zeros(B, num_iters, 3, FEATURES, dtype=torch.float64, device=device)
    for c in range(3):
        w[:, :, c, 6 + c] = 1.0
    return w


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
def color_correct_hip(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = DEFAULT_EPS) -> Tuple[Tensor, Tensor]:
    """gs_color_correct: img, ref [B,H,W,3] float32 on the GPU -> (corrected [B,H,W,3], warps float64 [B,num_iters,3,10])"""
    from . import _lib
    for t, name in ((img, "img"), (ref, "ref")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if img.dim() != 4 or img.shape[-1] != 3 or ref.shape != img.shape:
        raise ValueError("img and ref must both be [B,H,W,3]")
    if ref.device != img.device:
        raise ValueError("img and ref must live on the same device")
    if num_iters < 0:
        raise ValueError("num_iters must be >= 0")
    img, ref = img.contiguous(), ref.contiguous()
    B, H, W = (int(s) for s in img.shape[:3])
    out = torch.empty_like(img)
    warps = torch.empty(B, num_iters, 3, FEATURES, dtype=torch.float64, device=img.device)
    if B == 0 or H == 0 or W == 0:
        return out, warps
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(img.device):
        ws_bytes = int(lib.gs_color_correct_workspace_bytes(B, H, W))
        if ws_bytes < 0:
            raise _lib.HipLibraryError(f"color_correct: unsupported shape B={B}, H={H}, W={W}")
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=img.device)
        _lib.check(lib.gs_color_correct(B, H, W, vp(img.data_ptr()), vp(ref.data_ptr()), int(num_iters), float(eps),
                                        vp(out.data_ptr()), vp(warps.data_ptr()), vp(ws.data_ptr()), ws_bytes,
                                        vp(torch.cuda.current_stream().cuda_stream)), "color_correct")
    return out, warps


# --------------------------------------------------------------------------- #
# torch restatement (CPU tensors; the bench tool's baseline)
# --------------------------------------------------------------------------- #
def _features(x: Tensor) -> Tensor:
    r, g, b = x.unbind(-1)
    return torch.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, torch.ones_like(r)], dim=-1)


def _solve(G: Tensor, h: Tensor) -> Tuple[Tensor, Tensor]:
    """G [M,10,10], h [M,10] float64 -> (w [M,10], fitted [M] bool): Cholesky of the Jacobi-scaled matrix with the
    degenerate rule of colorcorrect_math.h solve_channel; rows that fail carry an arbitrary finite-or-not w"""
    n = FEATURES
    diag = G.diagonal(dim1=-2, dim2=-1)
    ok = (diag[:, n - 1] >= MIN_COUNT) & (diag > 0).all(-1)
    d = 1.0 / torch.where(diag > 0, diag, torch.ones_like(diag)).sqrt()
    S = G * d[:, :, None] * d[:, None, :]
    L = torch.zeros_like(S)
    for j in range(n):
        s = S[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
        good = s > PIVOT_TOL
        ok = ok & good
        ljj = torch.where(good, s, torch.ones_like(s)).sqrt()
        L[:, j, j] = ljj
        if j + 1 < n:
            L[:, j + 1:, j] = (S[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j:j + 1, :j]).sum(-1)) / ljj[:, None]
    y = torch.linalg.solve_triangular(L, (h * d)[..., None], upper=False)
    z = torch.linalg.solve_triangular(L.transpose(-1, -2), y, upper=True)[..., 0]
    return z * d, ok


def color_correct_torch(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = DEFAULT_EPS,
                        return_warps: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """the same algorithm as torch ops on img's device: float64 normal equations, float32 storage between iterations,
    float32 range tests, the degenerate rule.  [H,W,3] or [B,H,W,3]; warps float64 [(B,) num_iters, 3, 10]"""
    img4, ref4, single = _batched(img, ref)
    B, H, W = (int(s) for s in img4.shape[:3])
    dev = img4.device
    lo = torch.tensor(eps, dtype=torch.float32, device=dev)
    hi = torch.tensor(1.0 - eps, dtype=torch.float32, device=dev)
    fixed = (img4 >= lo) & (img4 <= hi) & (ref4 >= lo) & (ref4 <= hi)
    ref64 = ref4.double().reshape(B, H * W, 3)
    warps = identity_warps(B, num_iters, dev)
    x = img4.clone()
    for it in range(num_iters):
        mask = (fixed & (x >= lo) & (x <= hi)).reshape(B, H * W, 3)
        a = _features(x.double()).reshape(B, H * W, FEATURES)
        for c in range(3):
            am = (a * mask[..., c:c + 1]).transpose(1, 2)                      # [B,10,P], masked rows zeroed
            w, ok = _solve(am @ a, (am @ ref64[..., c:c + 1])[..., 0])
            warps[:, it, c] = torch.where(ok[:, None], w, warps[:, it, c])
        x = (a @ warps[:, it].transpose(1, 2)).clamp(0.0, 1.0).float().reshape(B, H, W, 3)
    if single:
        x, warps = x[0], warps[0]
    return (x, warps) if return_warps else x


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def color_correct(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = DEFAULT_EPS,
                  return_warps: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """Fit `img` to `ref` by a per-channel quadratic colour warp (module docstring) and return the fitted image, of img's
    shape: [H,W,3], or [B,H,W,3] for B independent pairs in one call.  float32 in [0,1].  return_warps: also the fitted
    weights, float64 [(B,) num_iters, 3, 10] (identity rows where the degenerate rule applied).  HIP tensors take the
    kernels, CPU tensors color_correct_torch.  No gradient: inputs that require grad are detached, the result is a
    constant."""
    img4, ref4, single = _batched(img, ref)
    if not img4.is_cuda:
        return color_correct_torch(img, ref, num_iters, eps, return_warps)
    out, warps = color_correct_hip(img4, ref4, num_iters, eps)
    if single:
        out, warps = out[0], warps[0]
    return (out, warps) if return_warps else out
