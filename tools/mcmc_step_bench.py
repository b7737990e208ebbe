"""What 3DGS-MCMC costs per training step on the MI355X (1M Gaussians): the noise step alone — gs_mcmc_inject_noise
against its torch restatement on the same GPU tensors, with the kernel's achieved bytes/s (56 B per Gaussian: 11 floats
read, 3 written) against the 8.0 TB/s peak —, gs_mcmc_relocation at M = 1 / 5 / 25 % of N, and a whole train_step with and
without inject_noise on bench.py's two scenes (1080p, S = 5).  Forms are alternated in blocks within one process.  One
JSON line, appended to profiles/mcmc_bench.jsonl with --record.

    python tools/mcmc_step_bench.py [--steps 20] [--blocks 3] [--warmup 3] [--gaussians 1000000] [--no-train] [--record]
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

PEAK_BYTES_PER_S = 8.0e12
BYTES_PER_ROW = 56


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


def kernels_only(gs, dev, N: int, steps: int, blocks: int, warmup: int) -> dict:
    import torch
    from gsdeblur_amd import mcmc
    g = torch.Generator(device=dev).manual_seed(0)
    means = torch.randn(N, 3, device=dev, generator=g)
    log_scales = torch.empty(N, 3, device=dev).uniform_(-6.0, -3.0, generator=g)
    quats = torch.randn(N, 4, device=dev, generator=g)
    logits = torch.empty(N, 1, device=dev).uniform_(-7.0, 4.0, generator=g)
    # a tiny scaler: the means stay put over many repetitions
    forms = {"noise_hip": lambda: mcmc.inject_noise_hip(means, log_scales, quats, logits, 1e-6, 0, 1),
             "noise_torch": lambda: mcmc.inject_noise_torch(means, log_scales, quats, logits, 1e-6, 0, 1)}
    keep = []
    for share in (0.01, 0.05, 0.25):
        M = int(N * share)
        o = torch.rand(M, device=dev, generator=g) * 0.99 + 0.005
        s = torch.exp(torch.empty(M, 3, device=dev).uniform_(-6.0, -3.0, generator=g))
        r = torch.randint(1, 8, (M,), device=dev, generator=g, dtype=torch.int32)
        keep.append((o, s, r))
        forms[f"relocation_{share * 100:g}pct"] = (lambda o=o, s=s, r=r: mcmc.relocation_hip(o, s, r))
    res = _alternate(forms, steps, blocks, warmup)
    out = {"N": N, **{k + "_ms": v["ms"] for k, v in res.items()}, "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}
    bps = BYTES_PER_ROW * N / (res["noise_hip"]["ms"] * 1e-3)
    out["noise_hip_bytes_per_s"] = round(bps, 1)
    out["noise_hip_share_of_8TBps_peak"] = round(bps / PEAK_BYTES_PER_S, 4)
    out["noise_torch_over_hip"] = round(res["noise_torch"]["ms"] / res["noise_hip"]["ms"], 2)
    return out


def train_iteration(gs, bench, dev, profile: str, N: int, W: int, H: int, S: int, steps: int, blocks: int,
                    warmup: int) -> dict:
    import torch
    from gsdeblur_amd import mcmc
    sc = bench.make_scene(N, W, H, profile=profile)
    c2w = torch.eye(4)[:3].clone()
    c2w[:, 1] *= -1
    c2w[:, 2] *= -1
    cam = gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                    metadata=dict(cam_idx=0, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * torch.tensor([1., -1., -1.])],
                                  camera_angular_velocity=[float(v) for v in sc["ang_vel"] * torch.tensor([1., -1., -1.])],
                                  exposure_time=sc["exposure_time"], rolling_shutter_time=0.0))
    target = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=S, rolling_shutter_compensation=False, gamma=2.2, min_rgb_level=10.0)
    mc = mcmc.MCMCConfig(noise_lr=1.0)              # a small noise: the scene stays the scene that is timed
    forms = {}
    for tag in ("train_step", "train_step_with_noise"):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
        opts = gs.training.make_optimizers(model)

        def step(m=model, o=opts, noise=tag.endswith("noise")):
            gs.training.train_step(m, o, cam, target, 0.2)
            if noise:
                mcmc.inject_noise(m, o, m.step, mc)
        forms[tag] = step
    res = _alternate(forms, steps, blocks, warmup)
    return {"scene": profile, "N": N, "size": [W, H], "S": S, **{k + "_ms": v["ms"] for k, v in res.items()},
            "blocks_ms": {k: v["blocks_ms"] for k, v in res.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per form, alternated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--no-train", action="store_true", help="the kernels alone")
    ap.add_argument("--record", action="store_true", help="append the result line to profiles/mcmc_bench.jsonl")
    args = ap.parse_args()

    import torch
    import gsdeblur_amd as gs
    import bench
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "kernels": kernels_only(gs, dev, args.gaussians, args.steps * 5, args.blocks, args.warmup)}
    torch.cuda.empty_cache()
    if not args.no_train:
        out["train_step"] = []
        for profile in ("survey", "trained"):
            out["train_step"].append(train_iteration(gs, bench, dev, profile, args.gaussians, 1920, 1080, 5, args.steps,
                                                     args.blocks, args.warmup))
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.record:
        with open(ROOT / "profiles" / "mcmc_bench.jsonl", "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
