"""What the normal terms cost per training step, and what the op costs alone: the headline scene (bench.py's 1M Gaussians,
1920x1080, S = 5 sub-poses) through render_step with the rgb gradient only (rgb), plus the depth-prior kernels
(fused_pearson), plus the normal kernels on the raw sums (normal_prior, normal_smooth, normal_both:
normals.normal_loss_with_grad, what train_step's normal_lambda / normal_smooth_lambda run).  The forms are alternated in
blocks within one process, so all see the same clocks, and the median block counts.  --op times the op alone on the scene's
sums: the kernels against normals.normal_loss_torch forced onto the same HIP tensors.  The line printed is JSON and is
appended to --out.

    python tools/normal_bench.py [--steps 30] [--blocks 4] [--warmup 5]
    python tools/normal_bench.py --op
    python tools/normal_bench.py --mode normal_both --steps 20      # one form only (for a rocprofv3 --kernel-trace --stats run)
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

FORMS = ("rgb", "fused_pearson", "normal_prior", "normal_smooth", "normal_both")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed steps per block")
    ap.add_argument("--blocks", type=int, default=4, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=("all",) + FORMS, default="all")
    ap.add_argument("--op", action="store_true", help="time the op alone: kernels against the torch form on HIP tensors")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "normal_bench.jsonl"), help="'' to only print")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    from gsdeblur_amd import normals as N
    from gsdeblur_amd.model import expected_depth
    dev = torch.device("cuda:0")
    S, H, W = 5, 1080, 1920
    wl = bench.Workload(gs, dev, 0, 1, 1_000_000, W, H, S, 1, "survey", "sparse")
    p, sc = wl.params, wl.sc
    intrins = (sc["fx"], sc["fy"], sc["cx"], sc["cy"])

    with torch.no_grad():
        rgb0, alphas, _, dacc = gs.render_combined(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"],
                                                   gs.subpose_viewmats(wl.viewmat, wl.lin, wl.ang, wl.times_t), wl.bg, S, 1,
                                                   sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2,
                                                   min_rgb_level=10.0, raw_params=True, return_depth=True, hints=wl.hints)
        d0 = expected_depth(dacc, alphas)
        depth_prior = torch.where(alphas.mean(dim=0)[..., None] > 0.5, d0 * 1.05, torch.zeros_like(d0)).reshape(H, W).contiguous()
        # the scene's own normals, tilted a little: a prior that is close and not equal
        prior = gs.depth_normals(dacc, alphas, intrins, 0.5)
        prior = torch.where((prior != 0).any(-1, keepdim=True), prior + 0.05, prior).contiguous()
        guide = rgb0.reshape(H, W, 3).clamp(0, 1).contiguous()

    def normal(prior_on, smooth_on):
        def grad_depth_sums(depth_acc, al):
            return gs.normal_loss_with_grad(depth_acc, al, intrins, prior if prior_on else None, guide if smooth_on else None,
                                            0.1 if prior_on else 0.0, 0.05 if smooth_on else 0.0, 2.0 if smooth_on else 0.0)[1:]
        return grad_depth_sums

    def pearson(depth_acc, al):
        return gs.depth_prior_loss_with_grad(depth_acc, al, depth_prior, "pearson", "depth", 0.1)[1:]

    callables = {"rgb": None, "fused_pearson": pearson, "normal_prior": normal(True, False),
                 "normal_smooth": normal(False, True), "normal_both": normal(True, True)}

    def step(form: str):
        gs.render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], wl.viewmat, wl.lin, wl.ang,
                       wl.times_t, wl.bg, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, wl.wt, gamma=2.2,
                       min_rgb_level=10.0, raw_params=True, hints=wl.hints, grad_depth=callables[form])

    def block(fn, n: int) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / n

    res = {"scene": "1M Gaussians, 1920x1080, S=5 (bench.py headline)", "steps_per_block": args.steps, "blocks": args.blocks}
    if args.op:
        kw = dict(prior=prior, guide=guide, prior_weight=0.1, smooth_weight=0.05, edge_beta=2.0)
        fns = {"op_hip": lambda: gs.normal_loss_with_grad(dacc, alphas, intrins, **kw),
               "op_torch_on_hip": lambda: N.normal_loss_torch(dacc, alphas, intrins, **kw)}
    else:
        forms = FORMS if args.mode == "all" else (args.mode,)
        fns = {f: (lambda f=f: step(f)) for f in forms}
    for fn in fns.values():
        block(fn, args.warmup)
    ms = {k: [] for k in fns}
    for _ in range(args.blocks):
        for k, fn in fns.items():
            ms[k].append(block(fn, args.steps))
    for k in fns:
        res[k + "_ms"] = round(statistics.median(ms[k]), 4)
        res[k + "_blocks_ms"] = [round(x, 4) for x in ms[k]]
    if "rgb" in fns:
        for k in fns:
            if k != "rgb":
                res[k + "_extra_ms"] = round(res[k + "_ms"] - res["rgb_ms"], 4)
    print(json.dumps(res))
    if args.out and (args.op or args.mode == "all"):
        with open(args.out, "at") as f:
            f.write(json.dumps({"tool": "normal_bench", **res}) + "\n")


if __name__ == "__main__":
    main()
