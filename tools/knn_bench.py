"""What the neighbour search behind from_seed_points costs on the MI355X: gs.knn (k = 3, default settings) per call at
N = 20k, 100k, 1M and 5M on a uniform cloud and on a clustered cloud (64 blobs, sigma 1 % of the cube) with 0.1 % far
outliers, with the number of rows the grid left to the brute-force kernel.  At N = 20k the route this replaces — the
tool's torch.cdist + topk on the same GPU tensors, which builds the N x N matrix — is timed beside it, alternated in
blocks, and the largest relative difference between the two results is reported (cdist's matmul form is inexact); at
the larger sizes only the allocation of that matrix is attempted and the outcome recorded.  One JSON line, appended to
profiles/knn_bench.jsonl with --record.

    python tools/knn_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--sizes 20000 100000 1000000 5000000] [--record]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CDIST_MAX_N = 20000            # the largest size at which the N x N route is timed (1.6 GB)


def _timed(fn, n: int) -> float:
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def _alternate(forms: dict, steps: int, blocks: int, warmup: int) -> dict:
    for f in forms.values():
        _timed(f, warmup)
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, f in forms.items():
            ms[k].append(_timed(f, steps))
    return {k: {"ms": round(statistics.median(v), 4), "blocks_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def cloud(kind: str, n: int, dev):
    import torch
    g = torch.Generator().manual_seed(17)
    if kind == "uniform":
        return torch.rand(n, 3, generator=g).to(dev)
    out = max(1, n // 1000)
    centres = torch.rand(64, 3, generator=g)
    pts = centres[torch.randint(0, 64, (n - out,), generator=g)] + 0.01 * torch.randn(n - out, 3, generator=g)
    far = 100.0 * torch.randn(out, 3, generator=g)
    return torch.cat([pts, far])[torch.randperm(n, generator=g)].contiguous().to(dev)


def cdist_topk(xyz):
    import torch
    d = torch.cdist(xyz, xyz)
    d.fill_diagonal_(float("inf"))
    return d.topk(3, largest=False).values


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed calls per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000, 1000000, 5000000])
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/knn_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    dev = torch.device("cuda:0")
    rows = []
    for kind in ("uniform", "clustered"):
        for n in args.sizes:
            xyz = cloud(kind, n, dev)
            d, stats = gs.knn(xyz, 3, return_stats=True)
            forms = {"knn": lambda: gs.knn(xyz, 3)}
            row = {"cloud": kind, "N": n, "k": 3, **stats, "fallback_share": round(stats["fallback_rows"] / n, 6)}
            if n <= CDIST_MAX_N:
                forms["cdist_topk"] = lambda: cdist_topk(xyz)
                ref = cdist_topk(xyz).sort(dim=1).values
                row["cdist_max_relative_difference"] = float(((ref - d).abs() / d.clamp(min=1e-30)).max())
                del ref
            else:
                # the route's first step is the N x N float32 matrix: only that allocation is attempted
                row["cdist_matrix_gb"] = round(4.0 * n * n / 1e9, 1)
                try:
                    torch.empty(n, n, dtype=torch.float32, device=dev)
                    row["cdist_topk"] = "not timed: the matrix alone allocates on this device"
                except RuntimeError as e:              # torch.OutOfMemoryError is one
                    row["cdist_topk"] = "cannot allocate: " + str(e).split("\n")[0][:160]
                torch.cuda.empty_cache()
            res = _alternate(forms, args.steps, args.blocks, args.warmup)
            row["knn_ms"] = res["knn"]["ms"]
            row["blocks_ms"] = {k: v["blocks_ms"] for k, v in res.items()}
            if "cdist_topk" in res:
                row["cdist_topk_ms"] = res["cdist_topk"]["ms"]
                row["cdist_over_knn"] = round(res["cdist_topk"]["ms"] / res["knn"]["ms"], 1)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del xyz, d
            torch.cuda.empty_cache()
    line = json.dumps({"device": torch.cuda.get_device_name(0), "knn": rows})
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "knn_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
