"""What a depth loss costs per training step: the headline scene (bench.py's 1M Gaussians, 1920x1080, S = 5 sub-poses)
through render_step with the rgb gradient only (rgb), with the rgb gradient plus an L1 loss on the expected depth as a
chain of torch ops (depth: the chain SplatfactoDeblurModel.render_and_backward runs: d loss / d depth -> d loss /
d depth_acc, d loss / d alphas), and with the depth-prior kernels on the raw sums in its place (fused_l1, fused_pearson:
depthprior.depth_prior_loss_with_grad, what train_step's depth_loss="l1" / "pearson" runs).  The forms are alternated in
blocks within one process, so all see the same clocks; the line printed is JSON and is appended to --out.

    python tools/depth_step_bench.py [--steps 30] [--blocks 4] [--warmup 5]              # rgb and depth
    python tools/depth_step_bench.py --mode all                                          # the four forms
    python tools/depth_step_bench.py --mode fused_pearson --steps 20   # one form only (for a rocprofv3 --kernel-trace --stats run)
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
    ap.add_argument("--mode", choices=("both", "all", "rgb", "depth", "fused_l1", "fused_pearson"), default="both")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_prior_bench.jsonl"),
                    help="--mode all appends its line here ('' to only print)")
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

    prior = gt.reshape(H, W).contiguous()

    def fused(kind):
        def grad_depth_sums(depth_acc, al):
            return gs.depth_prior_loss_with_grad(depth_acc, al, prior, kind, "depth", 0.1)[1:]
        return grad_depth_sums

    callables = {"rgb": None, "depth": grad_depth, "fused_l1": fused("l1"), "fused_pearson": fused("pearson")}

    def step(form: str):
        gs.render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], wl.viewmat, wl.lin, wl.ang,
                       wl.times_t, wl.bg, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, wl.wt, gamma=2.2,
                       min_rgb_level=10.0, raw_params=True, hints=wl.hints, grad_depth=callables[form])

    def block(form: str, n: int) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            step(form)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n

    forms = {"both": ("rgb", "depth"), "all": ("rgb", "depth", "fused_l1", "fused_pearson")}.get(args.mode, (args.mode,))
    for f in forms:
        block(f, args.warmup)
    ms = {f: [] for f in forms}
    for _ in range(args.blocks):
        for f in forms:
            ms[f].append(block(f, args.steps))
    res = {"scene": "1M Gaussians, 1920x1080, S=5 (bench.py headline)", "steps_per_block": args.steps,
           "blocks": args.blocks}
    keys = {"rgb": "rgb_only", "depth": "rgb_depth", "fused_l1": "rgb_fused_l1", "fused_pearson": "rgb_fused_pearson"}
    for f in forms:
        res[keys[f] + "_ms_per_step"] = round(statistics.median(ms[f]), 4)
        res[keys[f] + "_blocks_ms"] = [round(x, 4) for x in ms[f]]
    if args.mode == "both":
        res["ratio"] = round(res["rgb_depth_ms_per_step"] / res["rgb_only_ms_per_step"], 4)
    if args.mode == "all":
        for f in ("depth", "fused_l1", "fused_pearson"):
            res[keys[f] + "_extra_ms"] = round(res[keys[f] + "_ms_per_step"] - res["rgb_only_ms_per_step"], 4)
    print(json.dumps(res))
    if args.mode == "all" and args.out:
        with open(args.out, "at") as f:
            f.write(json.dumps({"tool": "depth_step_bench", **res}) + "\n")


if __name__ == "__main__":
    main()
