"""Reference and shared cases of the k-nearest-neighbour tests (tests/test_knn_host.py, tests/test_gpu_knn.py).

Reference: float64 ``torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist")`` on the float32 inputs, in chunks of
rows, the row itself excluded by index.  Nothing here calls the code under test.

Tolerance of every distance: rtol = 1e-6, atol = 0.  A float32 distance carries at most about 3.5 units of 2^-24 of
rounding (one subtraction, three squares, two additions, a square root); order statistics are 1-Lipschitz in the
perturbation, so a near-tie resolved differently moves a value by no more than that; a mean over k <= 16 adds at most k
units.  1e-6 is about 17 units.  Duplicates must give exactly 0 (atol = 0)."""
import functools
import struct

import torch

RTOL = 1e-6
CHUNK = 512


def reference(xyz, k, rows=None):
    """float64 [len(rows), k], ascending: the k smallest distances from each of `rows` (default: all) to the OTHER rows"""
    assert xyz.dtype == torch.float32
    x = xyz.detach().cpu().double()
    rows = torch.arange(x.shape[0]) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    out = torch.empty(len(rows), k, dtype=torch.float64)
    for lo in range(0, len(rows), CHUNK):
        r = rows[lo:lo + CHUNK]
        d = torch.cdist(x[r], x, compute_mode="donot_use_mm_for_euclid_dist")
        d[torch.arange(len(r)), r] = float("inf")
        out[lo:lo + CHUNK] = d.topk(k, dim=1, largest=False, sorted=True).values
    return out


def check_dists(got, ref, what=""):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    rel = float((err / ref.clamp(min=1e-300)).max())
    print(f"{what}: max relative error {rel:.2e} over {got.numel()} distances")
    assert bool((err <= RTOL * ref).all()), (what, rel)
    assert bool((got[ref == 0] == 0).all()), what
    assert bool((got[:, 1:] >= got[:, :-1]).all()), what


def check_indices(xyz, dists, idx, what=""):
    """distinct, never the row itself, and the float32 distance recomputed by the stated formula is the returned one"""
    xyz, dists, idx = xyz.detach().cpu(), dists.detach().cpu(), idx.detach().cpu().long()
    n, k = idx.shape
    assert idx.dtype == torch.int64 and bool((idx >= 0).all()) and bool((idx < n).all()), what
    assert bool((idx != torch.arange(n)[:, None]).all()), what
    s = idx.sort(dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all()), what
    d = xyz[:, None, :] - xyz[idx]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    # the correctly rounded float32 root (torch's float32 sqrt on the CPU is off by an ulp now and then): via float64
    again = ((dx * dx + dy * dy) + dz * dz).double().sqrt().float()
    assert torch.equal(again, dists), what


def open_rows_bound(kth, cell_size, max_rings):
    """how many rows the grid may leave to the brute-force kernel: those whose k-th distance exceeds R h (1 - 1e-6)"""
    return int((kth > max_rings * float(cell_size) * (1.0 - 1e-6)).sum())


def float_bits(i):
    return struct.unpack("<f", struct.pack("<i", int(i)))[0]


# ---- the shared clouds -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(n, seed=0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def lattice():
    r = torch.arange(5, dtype=torch.float32)
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def identical(n=8):
    return torch.tensor([[0.25, -1.5, 3.0]]).repeat(n, 1)


@functools.lru_cache(maxsize=None)
def clustered(far=False):
    """4000 points in four blobs (sigma 0.05 about (c, c, c), c = 0..3), 5 outliers of sigma 1e3; far: a sixth at 1e9"""
    g = torch.Generator().manual_seed(1)
    centres = torch.arange(4, dtype=torch.float32).repeat_interleave(1000)[:, None].expand(4000, 3)
    pts = torch.randn(4000, 3, generator=g) * 0.05 + centres
    out = torch.randn(5, 3, generator=g) * 1e3
    parts = [pts, out] + ([torch.tensor([[1e9, -1e9, 1e9]])] if far else [])
    return torch.cat(parts).contiguous()


@functools.lru_cache(maxsize=None)
def cached_reference(name, *args, k=3):
    return reference(globals()[name](*args), k)
