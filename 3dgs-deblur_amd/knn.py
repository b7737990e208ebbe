"""Exact k nearest neighbours of a point cloud against itself: what splatfacto's initialisation needs (the scale of a
Gaussian started from a seed cloud is the mean distance to its 3 nearest neighbours) at the size of a real capture, where
the N x N distance matrix of ``torch.cdist`` + ``topk`` cannot be built (40 GB at 100k points).

For every row i: the k smallest (squared distance, index) pairs over the rows j != i.  A row is excluded by index, so a
duplicate point is a neighbour at distance 0.  The squared distance is ``(dx*dx + dy*dy) + dz*dz`` with ``dx = x_i - x_j``
in float32, every operation rounded; the returned distance is its correctly rounded float32 square root (torch's own
float32 sqrt is not always: the root is taken in float64 and rounded).  The pair order is total (ties in
the squared distance go to the smaller index), so distances AND indices are deterministic and do not depend on the order
of the rows, block shapes or scheduling.  csrc/knn_math.h states the algorithm — a hashed uniform grid walked in Chebyshev
shells, with a brute-force kernel for the rows the grid leaves open — and why it is exact.

On HIP tensors the kernels of csrc/knn.hip are the only route (``gs_knn``: one call, nothing read back, no float atomics,
memory linear in N); CPU tensors take ``knn_torch``, a chunked brute force of the same rules as torch ops.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

MAX_K = 16                           # csrc/knn_math.h kMaxK
DEFAULT_MAX_RINGS = 8                # kDefaultMaxRings
MAX_N = 1 << 26                      # kMaxN
_CHUNK_ELEMS = 1 << 22               # knn_torch: rows x N distances per chunk


def _check(xyz: Tensor, k: int) -> None:
    if not isinstance(xyz, Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be [N,3], got {tuple(getattr(xyz, 'shape', ()))}")
    if xyz.dtype != torch.float32:
        raise ValueError(f"xyz must be float32, got {xyz.dtype}")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    if xyz.shape[0] <= k:
        raise ValueError(f"knn needs more than k = {k} rows, got {xyz.shape[0]}")
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("xyz must be finite")


# --------------------------------------------------------------------------- #
# HIP
# --------------------------------------------------------------------------- #
def knn_hip(xyz: Tensor, k: int = 3, cell_size: float = 0.0, max_rings: int = 0,
            want_indices: bool = False, want_stats: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """gs_knn: xyz [N,3] float32 on the GPU -> (dists [N,k] float32, idx [N,k] int32 or None, stats int32 [4] on the
    device or None).  cell_size <= 0: chosen on the device; max_rings <= 0: the default"""
    from . import _lib
    if not xyz.is_cuda:
        raise ValueError("xyz must be a CUDA(HIP) tensor: the HIP path has no CPU fallback")
    _check(xyz, k)
    xyz = xyz.detach().contiguous()
    N, k = int(xyz.shape[0]), int(k)
    if N > MAX_N:
        raise ValueError(f"knn supports at most {MAX_N} rows, got {N}")
    dists = torch.empty(N, k, dtype=torch.float32, device=xyz.device)
    idx = torch.empty(N, k, dtype=torch.int32, device=xyz.device) if want_indices else None
    stats = torch.empty(4, dtype=torch.int32, device=xyz.device) if want_stats else None
    lib = _lib.load()
    vp = ctypes.c_void_p
    with torch.cuda.device(xyz.device):
        ws_bytes = int(lib.gs_knn_workspace_bytes(N, k))
        if ws_bytes < 0:
            raise _lib.HipLibraryError(f"knn: unsupported shape N={N}, k={k}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xyz.device)
        _lib.check(lib.gs_knn(N, vp(xyz.data_ptr()), k, float(cell_size or 0.0), int(max_rings or 0), vp(dists.data_ptr()),
                              vp(idx.data_ptr()) if want_indices else None, vp(stats.data_ptr()) if want_stats else None,
                              vp(ws.data_ptr()), ws_bytes, vp(torch.cuda.current_stream().cuda_stream)), "knn")
    return dists, idx, stats


def _stats_dict(stats: Tensor) -> Dict:
    s = [int(v) for v in stats.tolist()]
    return {"cell_size": struct.unpack("<f", struct.pack("<i", s[0]))[0], "max_rings": s[1], "fallback_rows": s[2],
            "table_bits": s[3]}


# --------------------------------------------------------------------------- #
# torch restatement (CPU tensors)
# --------------------------------------------------------------------------- #
def knn_torch(xyz: Tensor, k: int = 3, return_indices: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """the same result as torch ops on xyz's device: brute force in chunks of rows (rows x N distances at a time, never
    N x N), the squared distance formed as the kernels form it, a stable sort so that ties go to the smaller index"""
    _check(xyz, k)
    xyz = xyz.detach()
    N = int(xyz.shape[0])
    x, y, z = (xyz[:, a].contiguous() for a in range(3))
    dists = torch.empty(N, k, dtype=torch.float32, device=xyz.device)
    idx = torch.empty(N, k, dtype=torch.int64, device=xyz.device)
    rows = max(1, _CHUNK_ELEMS // N)
    for lo in range(0, N, rows):
        hi = min(N, lo + rows)
        dx, dy, dz = x[lo:hi, None] - x[None, :], y[lo:hi, None] - y[None, :], z[lo:hi, None] - z[None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[torch.arange(hi - lo), torch.arange(lo, hi)] = float("inf")       # the row itself, by index
        v, i = torch.sort(d2, dim=1, stable=True)
        dists[lo:hi], idx[lo:hi] = v[:, :k].double().sqrt().float(), i[:, :k]      # the correctly rounded root
    return (dists, idx.to(torch.int32)) if return_indices else dists


# --------------------------------------------------------------------------- #
# public surface
# --------------------------------------------------------------------------- #
def knn(xyz: Tensor, k: int = 3, return_indices: bool = False, return_stats: bool = False,
        cell_size: Optional[float] = None, max_rings: Optional[int] = None):
    """Distances [N,k] float32, ascending, from every row of xyz [N,3] float32 to its k nearest OTHER rows (module
    docstring); exact.  return_indices: also their rows, int32 [N,k].  return_stats: also a dict with cell_size,
    max_rings, fallback_rows (rows the grid left to the brute-force kernel) and table_bits; on CPU tensors, which take
    knn_torch and have no grid, cell_size is 0.0 and fallback_rows is N.  cell_size / max_rings override the choices
    of the HIP path (tests, tuning) and never change the result.  ValueError for N <= k, k outside 1..16, non-finite input,
    a wrong shape or dtype.  No gradient."""
    if not isinstance(xyz, Tensor):
        raise ValueError("xyz must be a tensor")
    if cell_size is not None and not float(cell_size) > 0.0:
        raise ValueError("cell_size must be positive")
    if max_rings is not None and int(max_rings) < 1:
        raise ValueError("max_rings must be at least 1")
    if xyz.is_cuda:
        dists, idx, stats = knn_hip(xyz, k, cell_size or 0.0, max_rings or 0, return_indices, return_stats)
        info = _stats_dict(stats) if return_stats else None
    else:
        out = knn_torch(xyz, k, return_indices)
        dists, idx = out if return_indices else (out, None)
        info = {"cell_size": 0.0, "max_rings": int(max_rings or DEFAULT_MAX_RINGS), "fallback_rows": int(xyz.shape[0]),
                "table_bits": 0}
    res = (dists,) + ((idx,) if return_indices else ()) + ((info,) if return_stats else ())
    return res[0] if len(res) == 1 else res


def knn_mean_distance(xyz: Tensor, k: int = 3) -> Tensor:
    """[N]: the mean distance of every row to its k nearest other rows"""
    return knn(xyz, k).mean(dim=1)


# the package exports the function under the module's name (gs.knn): its siblings stay reachable through it
knn.knn_torch = knn_torch
knn.knn_hip = knn_hip
knn.knn_mean_distance = knn_mean_distance
