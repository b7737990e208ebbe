"""What the per-frame blur statistics cost on the MI355X: gs.blur_stats (csrc/blur.hip) per call at (frames, points) =
(200, 100k) and (1000, 1M) beside blur_stats_torch — the same operations as torch ops on the same GPU tensors, chunked
over frames — alternated in blocks, with the largest relative difference between the two results; and the sweep of the
points a thread keeps in registers (1, 2, 4, 8, 16 at a fixed chunk of 1024 points per workgroup) that the library's
default was chosen from.  Pair rates are frames x points / time.  One JSON line, appended to
profiles/blur_score_bench.jsonl with --record.

    python tools/blur_score_bench.py [--steps 5] [--blocks 3] [--warmup 2] [--shapes 200x100000 1000x1000000] [--record]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PPTS = (1, 2, 4, 8, 16)
W, H, FOCAL = 1920, 1080, 1500.0


def _timed(fn, n: int) -> float:
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def _alternate(forms: dict, steps: dict, blocks: int, warmup: int) -> dict:
    for k, f in forms.items():
        _timed(f, min(warmup, steps[k]))
    ms = {k: [] for k in forms}
    for _ in range(blocks):
        for k, f in forms.items():
            ms[k].append(_timed(f, steps[k]))
    return {k: {"ms": round(statistics.median(v), 4), "blocks_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def scene(F: int, N: int, dev):
    """N points uniform in a 6 m cube, F cameras on a circle of radius 8 m looking at its centre, seeded twists"""
    import torch
    g = torch.Generator().manual_seed(23)
    pts = (torch.rand(N, 3, generator=g) * 6.0 - 3.0)
    th = 2 * math.pi * torch.arange(F, dtype=torch.float64) / F
    eye = torch.stack([8.0 * torch.cos(th), 0.5 * torch.sin(3 * th), 8.0 * torch.sin(th)], 1)
    z = -eye / eye.norm(dim=1, keepdim=True)
    x = torch.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand(F, 3), z, dim=1)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.cross(z, x, dim=1)
    Rm = torch.stack([x, y, z], 1)
    V = torch.eye(4, dtype=torch.float64).repeat(F, 1, 1)
    V[:, :3, :3] = Rm
    V[:, :3, 3] = -(Rm @ eye[:, :, None])[:, :, 0]
    lin = torch.rand(F, 3, generator=g) - 0.5
    ang = (torch.rand(F, 3, generator=g) - 0.5) * 1.2
    intr = torch.tensor([FOCAL, FOCAL, W / 2.0, H / 2.0]).repeat(F, 1)
    times = torch.tensor([0.02, 0.03]).repeat(F, 1)
    return [t.float().contiguous().to(dev) for t in (pts, V, lin, ang, intr, times)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed calls per block (the torch form: 1)")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=["200x100000", "1000x1000000"], help="FRAMESxPOINTS")
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/blur_score_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    from gsdeblur_amd.blurscore import blur_stats_hip, blur_stats_torch
    dev = torch.device("cuda:0")
    rows = []
    for shape in args.shapes:
        F, N = (int(v) for v in shape.lower().split("x"))
        t = scene(F, N, dev)
        got, ref = gs.blur_stats(*t, W, H), blur_stats_torch(*t, W, H)
        row = {"F": F, "N": N, "pairs": F * N, "visible_share": round(float(got.count.double().mean()) / N, 4),
               "counts_equal": bool(torch.equal(got.count, ref.count)),
               "max_relative_difference": max(float(((getattr(got, k) - getattr(ref, k)).abs()
                                                     / getattr(ref, k).abs().clamp(min=1e-30)).max())
                                              for k in ("mean_blur", "rms_blur", "max_blur", "mean_skew"))}
        forms = {"hip": lambda: gs.blur_stats(*t, W, H), "torch": lambda: blur_stats_torch(*t, W, H)}
        steps = {"hip": args.steps, "torch": 1}
        for p in PPTS:
            forms[f"ppt{p}"] = (lambda p=p: blur_stats_hip(*t, W, H, points_per_thread=p))
            steps[f"ppt{p}"] = args.steps
        res = _alternate(forms, steps, args.blocks, args.warmup)
        row["hip_ms"], row["torch_ms"] = res["hip"]["ms"], res["torch"]["ms"]
        row["torch_over_hip"] = round(res["torch"]["ms"] / res["hip"]["ms"], 1)
        row["hip_gpairs_per_s"] = round(F * N / res["hip"]["ms"] / 1e6, 2)
        row["points_per_thread_ms"] = {str(p): res[f"ppt{p}"]["ms"] for p in PPTS}
        row["blocks_ms"] = {k: v["blocks_ms"] for k, v in res.items()}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del t, got, ref
        torch.cuda.empty_cache()
    line = json.dumps({"device": torch.cuda.get_device_name(0), "image": [W, H], "blur_stats": rows})
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "blur_score_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
