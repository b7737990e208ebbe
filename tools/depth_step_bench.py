"""What a depth loss costs per training step: the headline scene (bench.py's 1M Gaussians, 1920x1080, S = 5 sub-poses)
through render_step with the rgb gradient only, and with the rgb gradient plus an L1 loss on the expected depth (the chain
SplatfactoDeblurModel.render_and_backward runs: d loss / d depth -> d loss / d depth_acc, d loss / d alphas).  The two
forms are alternated in blocks within one process, so both see the same clocks; the line printed is JSON.

    python tools/depth_step_bench.py [--steps 30] [--blocks 4] [--warmup 5]
    python tools/depth_step_bench.py --mode depth --steps 20   # one form only (for a rocprofv3 --kernel-trace --stats run)
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=4, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "rgb", "depth"), default="both")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    from gsdeblur_amd.model import expected_depth
    dev = torch.device("cuda:0")
    S, H, W = 5, 1080, 1920
    wl = bench.Workload(gs, dev, 0, 1, 1_000_000, W, H, S, 1, "survey", "sparse")
    p, sc = wl.params, wl.sc

    # ground-truth depth: the scene's own expected depth, scaled by 1.05 where a pixel is covered (0 = no measurement)
    with torch.no_grad():
        _, alphas, _, dacc = gs.render_combined(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"],
                                                gs.subpose_viewmats(wl.viewmat, wl.lin, wl.ang, wl.times_t), wl.bg, S, 1,
                                                sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                                                min_rgb_level=10.0, raw_params=True, return_depth=True, hints=wl.hints)
        d0 = expected_depth(dacc, alphas)
        gt = torch.where(alphas.mean(dim=0)[..., None] > 0.5, d0 * 1.05, torch.zeros_like(d0))
    n_valid = float((gt > 0).sum().clamp(min=1))

    def grad_depth(depth_acc, al):
        da, a = depth_acc.requires_grad_(True), al.requires_grad_(True)
        depth = expected_depth(da, a)
        loss = 0.1 * ((depth - gt).abs() * (gt > 0)).sum() / n_valid
        return torch.autograd.grad(loss, (da, a), allow_unused=True)

    def step(depth: bool):
        gs.render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], wl.viewmat, wl.lin, wl.ang,
                       wl.times_t, wl.bg, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, wl.wt, gamma=2.2,
                       min_rgb_level=10.0, raw_params=True, hints=wl.hints, grad_depth=grad_depth if depth else None)

    def block(depth: bool, n: int) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            step(depth)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n

    forms = {"both": (False, True), "rgb": (False,), "depth": (True,)}[args.mode]
    for f in forms:
        block(f, args.warmup)
    ms = {f: [] for f in forms}
    for _ in range(args.blocks):
        for f in forms:
            ms[f].append(block(f, args.steps))
    res = {"scene": "1M Gaussians, 1920x1080, S=5 (bench.py headline)", "steps_per_block": args.steps,
           "blocks": args.blocks}
    for f in forms:
        key = "rgb_depth" if f else "rgb_only"
        res[key + "_ms_per_step"] = round(statistics.median(ms[f]), 4)
        res[key + "_blocks_ms"] = [round(x, 4) for x in ms[f]]
    if len(forms) == 2:
        res["ratio"] = round(res["rgb_depth_ms_per_step"] / res["rgb_only_ms_per_step"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
