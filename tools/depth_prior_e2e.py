"""Does a depth PRIOR that is not metric recover geometry?  The construction of
tests/test_gpu_depth_grad.py::test_depth_supervision_recovers_geometry_end_to_end — a seeded synthetic scene, ground-truth
rgb and depth rendered by the library from 8 views, the model started from the same Gaussians with their means pushed
along the rays — but the trainer is handed priors in arbitrary units: 0.37 * depth + 1.9 (depth space) and 2 / depth + 0.1
(disparity space), with train_step's depth_loss="pearson".  Trained with depth_lambda = 0 and with the prior term on the
same schedule; reported: the held-out METRIC depth L1 against the true depth and the held-out PSNR.

    python tools/depth_prior_e2e.py [--steps 1000] [--depth-lambda 0.5]      # appends to profiles/depth_prior_train.jsonl
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PRIORS = {"depth": lambda d: 0.37 * d + 1.9, "disparity": lambda d: 2.0 / d + 0.1}


def views(gs, sc, W, H, n_views):
    """n_views pinhole cameras around the scene's own (OpenGL camera-to-world, no motion): a small orbit of positions"""
    import torch
    cams = []
    for v in range(n_views):
        c2w = torch.eye(4)[:3].clone()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        ph = 2.0 * math.pi * v / n_views
        c2w[:, 3] = torch.tensor([0.25 * math.cos(ph), 0.15 * math.sin(ph), 0.0])
        cams.append(gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W, H,
                              metadata=dict(cam_idx=v, camera_linear_velocity=[0.0, 0.0, 0.0],
                                            camera_angular_velocity=[0.0, 0.0, 0.0], exposure_time=0.0,
                                            rolling_shutter_time=0.0)))
    return cams


def held_out_depth_l1(model, cams, depths, idx):
    errs = []
    for i in idx:
        out = model.get_outputs_for_camera(cams[i])
        valid = depths[i] > 0
        errs.append(float((out["depth"] - depths[i]).abs()[valid].mean()))
    return sum(errs) / len(errs)


def run(gs, dev, steps: int = 300, depth_lambda: float = 0.5, spaces=("depth", "disparity"), depth_loss: str = "pearson",
        n: int = 3000, W: int = 128, H: int = 96):
    """-> {"none": (held-out depth L1, PSNR), "depth": ..., "disparity": ...}: one run without a depth term, one per space
    with the non-metric prior of that space"""
    import torch
    from gsdeblur_amd import training as T
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=77)
    cams = views(gs, sc, W, H, 8)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=0, rolling_shutter_compensation=False, gamma=1.0)
    gt_model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    images, depths = [], []
    with torch.no_grad():
        for c in cams:
            out = gt_model.get_outputs_for_camera(c)
            images.append(out["rgb"].clamp(0, 1).contiguous())
            depths.append(torch.where(out["accumulation"] > 0.5, out["depth"], torch.zeros_like(out["depth"])).contiguous())
    g = torch.Generator().manual_seed(78)
    push = (torch.rand(n, 1, generator=g) * 0.3 + 0.15) * torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    start = dict(sc)
    start["means"] = sc["means"] * (1.0 + push)                       # along the ray through the camera centre (0, 0, 0)
    start["log_scales"] = sc["log_scales"] + torch.log1p(push)
    scene = types.SimpleNamespace(cameras=cams, train_indices=[1, 2, 3, 5, 6, 7], eval_indices=[0, 4])
    res = {}
    for name in ("none",) + tuple(spaces):
        model = gs.SplatfactoDeblurModel.from_scene(cfg, start, dev)
        torch.manual_seed(0)
        if name == "none":
            r = T.train_scene(model, scene, images, steps, depths=depths, depth_lambda=0.0, seed=3)
        else:
            # what the trainer sees is NOT metric: an affine map of the depth, or of its inverse; 0 stays "no value"
            priors = [torch.where(d > 0, PRIORS[name](d), torch.zeros_like(d)).contiguous() for d in depths]
            r = T.train_scene(model, scene, images, steps, depths=priors, depth_lambda=depth_lambda, seed=3,
                              depth_loss=depth_loss, depth_space=name)
        res[name] = (held_out_depth_l1(model, cams, depths, scene.eval_indices), r["results"]["psnr"])
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--depth-lambda", type=float, default=0.5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "depth_prior_train.jsonl"))
    args = ap.parse_args()
    import torch
    import gsdeblur_amd as gs
    dev = torch.device("cuda:0")
    t0 = time.time()
    res = run(gs, dev, args.steps, args.depth_lambda)
    line = {"tool": "depth_prior_e2e", "scene": "3000 Gaussians, 128x96, 8 views (6 train, 2 held out), means pushed along the rays",
            "steps": args.steps, "depth_lambda": args.depth_lambda, "depth_loss": "pearson",
            "held_out_depth_l1_none": round(res["none"][0], 4), "held_out_psnr_none": round(res["none"][1], 3)}
    for space in ("depth", "disparity"):
        line[f"prior_{space}"] = "0.37*depth+1.9" if space == "depth" else "2/depth+0.1"
        line[f"held_out_depth_l1_{space}"] = round(res[space][0], 4)
        line[f"depth_l1_ratio_{space}"] = round(res[space][0] / res["none"][0], 4)
        line[f"held_out_psnr_{space}"] = round(res[space][1], 3)
    line["seconds"] = round(time.time() - t0, 1)
    print(json.dumps(line))
    with open(args.out, "at") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
