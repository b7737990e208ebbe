"""What the colour fit behind cc_psnr / cc_ssim costs per evaluation image on the MI355X: gs_color_correct (five
iterations in one call) against color_correct_torch — the float64 normal equations as torch ops, the form the kernels
replace — on the same GPU tensors, at 480 x 270 and 1920 x 1080, for B = 1 and B = 8 image pairs per call.  The pictures
are a smooth colour field plus noise with a few saturated pixels and a mild colour warp between image and reference (what
a render and its ground truth are).  Forms are alternated in blocks within one process.  One JSON line, appended to
profiles/color_correct_bench.jsonl with --record.

    python tools/color_correct_bench.py [--steps 3] [--blocks 3] [--warmup 1] [--record]
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

SIZES = ((480, 270), (1920, 1080))
BATCHES = (1, 8)


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


def _pair(B: int, H: int, W: int, dev):
    import torch
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    ref = torch.stack([0.15 + 0.7 * xx, 0.2 + 0.6 * yy, 0.5 + 0.3 * torch.sin(6 * xx + 3 * yy)], dim=-1)
    ref = (ref[None] + 0.05 * torch.randn(B, H, W, 3, generator=g)).clamp(0, 1)
    img = (ref * torch.tensor([0.85, 1.0, 1.1]) + 0.03 * ref * ref + 0.01 * torch.randn(B, H, W, 3, generator=g)).clamp(0, 1)
    return img.to(dev).contiguous(), ref.to(dev).contiguous()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/color_correct_bench.jsonl")
    args = ap.parse_args()

    import torch
    from gsdeblur_amd import colorcorrect as CC
    dev = torch.device("cuda:0")
    rows = []
    for W, H in SIZES:
        for B in BATCHES:
            img, ref = _pair(B, H, W, dev)
            diff = float((CC.color_correct_hip(img, ref)[0] - CC.color_correct_torch(img, ref)).abs().max())
            res = _alternate({"hip": lambda: CC.color_correct_hip(img, ref),
                              "torch": lambda: CC.color_correct_torch(img, ref)}, args.steps, args.blocks, args.warmup)
            rows.append({"size": [W, H], "B": B, "num_iters": 5, "hip_ms": res["hip"]["ms"], "torch_ms": res["torch"]["ms"],
                         "hip_ms_per_image": round(res["hip"]["ms"] / B, 4),
                         "torch_over_hip": round(res["torch"]["ms"] / res["hip"]["ms"], 1),
                         "max_abs_difference": diff, "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)     # progress: the torch form takes seconds per call
            del img, ref
            torch.cuda.empty_cache()
    line = json.dumps({"device": torch.cuda.get_device_name(0), "color_correct": rows})
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "color_correct_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
