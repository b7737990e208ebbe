"""What the camera-shutter optimizer costs per training step on the MI355X: a whole train_step with the optimizer off
(the step of the commit before the feature: the cached host schedule, gs_subpose_viewmats_bwd_store, no new parameter or
launch) and on (exposure + readout "global": ops.subpose_times' handful of scalar torch ops, the 19-tangent sub-pose
backward gs_subpose_viewmats_bwd_times, one more dense Adam group) on bench.py's two scenes — the headline-like "survey"
profile and the fitted-model-like "trained" one — at 1080p, S = 5, R = 2.  Forms are alternated in blocks within one
process.  One JSON line, appended to profiles/shutter_step_bench.jsonl with --record.

    python tools/shutter_step_bench.py [--steps 20] [--blocks 3] [--warmup 3] [--gaussians 1000000] [--record]
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


def train_iteration(gs, bench, dev, profile: str, N: int, W: int, H: int, S: int, R: int, steps: int, blocks: int,
                    warmup: int) -> dict:
    import torch
    sc = bench.make_scene(N, W, H, profile=profile)
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    flip = torch.tensor([1., -1., -1.])
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * flip],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * flip],
                                  exposure_time=sc["exposure_time"], rolling_shutter_time=sc["exposure_time"]))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    forms = {}
    for tag, on in (("train_step", False), ("train_step_with_shutter_opt", True)):
        cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=R > 1, rs_bands=R, gamma=2.2,
                                        min_rgb_level=10.0)
        if on:
            cfg.camera_shutter_optimizer.exposure = cfg.camera_shutter_optimizer.readout = "global"
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=1)
        opts = gs.training.make_optimizers(model, lr_scale=1e-3)      # the scene stays the scene that is timed
        forms[tag] = (lambda m=model, o=opts: gs.training.train_step(m, o, cam, target, 0.2))
    res = _alternate(forms, steps, blocks, warmup)
    return {"scene": profile, "N": N, "size": [W, H], "S": S, "R": R, **{k + "_ms": v["ms"] for k, v in res.items()},
            "shutter_cost_ms": round(res["train_step_with_shutter_opt"]["ms"] - res["train_step"]["ms"], 4),
            "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/shutter_step_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "train_step": []}
    for profile in ("survey", "trained"):
        out["train_step"].append(train_iteration(gs, bench, dev, profile, args.gaussians, 1920, 1080, 5, 2, args.steps,
                                                 args.blocks, args.warmup))
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "shutter_step_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
