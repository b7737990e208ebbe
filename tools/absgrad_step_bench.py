"""What the absgrad statistic costs per training step: render_step on bench.py's scenes (1M Gaussians, 1920x1080, S = 5
sub-poses; profile "survey" = the headline scene, "trained" = the fitted-model-like one) with xy_grad_out only and with
xy_absgrad_out as well.  The two forms are alternated in blocks within one process, so both see the same clocks.  A
second pass times the backward compositor alone with the library's own HIP events (stage raster_bwd), again alternated.
One JSON line per scene, appended to profiles/absgrad_bench.jsonl with --record.

    python tools/absgrad_step_bench.py [--steps 30] [--blocks 4] [--warmup 5] [--scenes survey,trained] [--record]
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
    ap.add_argument("--scenes", default="survey,trained")
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--record", action="store_true", help="append the result lines to profiles/absgrad_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    from gsdeblur_amd import ops
    from gsdeblur_amd._profile import StageProfiler
    dev = torch.device("cuda:0")
    S, H, W = 5, 1080, 1920
    for profile in args.scenes.split(","):
        wl = bench.Workload(gs, dev, 0, 1, args.gaussians, W, H, S, 1, profile, "sparse")
        p, sc = wl.params, wl.sc
        n = p["means"].shape[0]
        xy = torch.zeros(n, 2, device=dev)
        xa = torch.empty(n, 2, device=dev)

        def step(absgrad: bool):
            gs.render_step(p["means"], p["log_scales"], p["quats"], p["opacity_logits"], p["sh"], wl.viewmat, wl.lin,
                           wl.ang, wl.times_t, wl.bg, S, 1, sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, wl.wt,
                           gamma=2.2, min_rgb_level=10.0, raw_params=True, hints=wl.hints, xy_grad_out=xy,
                           xy_absgrad_out=xa if absgrad else None)

        def block(absgrad: bool, k: int) -> float:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(k):
                step(absgrad)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3 / k

        forms = (False, True)
        for f in forms:
            block(f, args.warmup)
        ms = {f: [] for f in forms}
        for _ in range(args.blocks):
            for f in forms:
                ms[f].append(block(f, args.steps))
        # the backward compositor alone: the library's HIP events around its launches (summed over a step's slices)
        kern = {f: [] for f in forms}
        for _ in range(args.blocks):
            for f in forms:
                ops.profiler = StageProfiler(only=("raster_bwd",))
                try:
                    for _ in range(args.steps):
                        step(f)
                    per = ops.profiler.summary_ms().get("raster_bwd", [])
                finally:
                    ops.profiler = None
                kern[f].append(sum(per) / args.steps)
        res = {"scene": f"{n} Gaussians, {W}x{H}, S={S}, profile {profile!r}", "steps_per_block": args.steps,
               "blocks": args.blocks, "device": torch.cuda.get_device_name(0)}
        for f in forms:
            key = "absgrad_on" if f else "absgrad_off"
            res[key + "_ms_per_step"] = round(statistics.median(ms[f]), 4)
            res[key + "_blocks_ms"] = [round(x, 4) for x in ms[f]]
            res[key + "_raster_bwd_ms"] = round(statistics.median(kern[f]), 4)
            res[key + "_raster_bwd_blocks_ms"] = [round(x, 4) for x in kern[f]]
        res["step_ratio"] = round(res["absgrad_on_ms_per_step"] / res["absgrad_off_ms_per_step"], 4)
        res["raster_bwd_ratio"] = round(res["absgrad_on_raster_bwd_ms"] / res["absgrad_off_raster_bwd_ms"], 4)
        line = json.dumps(res)
        print(line, flush=True)
        if args.record:
            with open(ROOT / "profiles" / "absgrad_bench.jsonl", "a") as fh:
                fh.write(line + "\n")
        del wl, p, xy, xa
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
