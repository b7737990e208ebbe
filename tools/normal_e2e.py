"""Do normal priors, and normal smoothness alone, recover surface orientation?  The construction of
tools/depth_prior_e2e.py — a seeded synthetic scene, ground-truth rgb rendered by the library from 8 views, the model
started from the same Gaussians with their means pushed along the rays — with normal priors that are gs.depth_normals of
the TRUE scene's rendered depth.  Trained without the term, with the prior term (plus smoothness), and with smoothness
alone, on the same schedule; reported for the two held-out views: the mean angle between the trained model's
depth-derived normals and the true scene's (over the pixels where both exist), the metric depth L1 and the PSNR.

    python tools/normal_e2e.py [--steps 1000] [--normal-lambda 0.02]      # appends to profiles/normal_train.jsonl
"""
from __future__ import annotations

import argparse
import json
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

VARIANTS = {                  # name: (prior on, smoothness on)
    "none": (False, False), "prior": (True, False), "prior_smooth": (True, True), "smooth": (False, True),
}


def held_out_angle(model, cams, true_normals, idx, min_alpha=0.5):
    """mean angle in degrees between model.render_normals and the true normals, over the pixels where both exist"""
    import torch
    angles = []
    for i in idx:
        n = model.render_normals(cams[i], sharp=False, min_alpha=min_alpha)
        both = (n != 0).any(-1) & (true_normals[i] != 0).any(-1)
        cos = (n * true_normals[i]).sum(-1)[both].clamp(-1.0, 1.0)
        angles.append(float(torch.rad2deg(torch.acos(cos)).mean()))
    return sum(angles) / len(angles)


def run(gs, dev, steps: int = 300, normal_lambda: float = 0.02, smooth_lambda: float = 0.01, edge_beta: float = 0.0,
        variants=("none", "prior_smooth", "smooth"), n: int = 3000, W: int = 128, H: int = 96):
    """-> {variant: (held-out normal angle in degrees, held-out depth L1, PSNR)}"""
    import torch
    from depth_prior_e2e import held_out_depth_l1, views
    from gsdeblur_amd import training as T
    sc = gs.data.synthetic_scene(n, W, H, sh_degree=3, seed=77)
    cams = views(gs, sc, W, H, 8)
    cfg = gs.SplatfactoDeblurConfig(blur_samples=0, rolling_shutter_compensation=False, gamma=1.0)
    gt_model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev)
    images, depths, normals = [], [], []
    with torch.no_grad():
        for c in cams:
            out = gt_model.get_outputs_for_camera(c)
            images.append(out["rgb"].clamp(0, 1).contiguous())
            depths.append(torch.where(out["accumulation"] > 0.5, out["depth"], torch.zeros_like(out["depth"])).contiguous())
            normals.append(gt_model.render_normals(c, sharp=False, min_alpha=0.5))
    g = torch.Generator().manual_seed(78)
    push = (torch.rand(n, 1, generator=g) * 0.3 + 0.15) * torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    start = dict(sc)
    start["means"] = sc["means"] * (1.0 + push)                       # along the ray through the camera centre (0, 0, 0)
    start["log_scales"] = sc["log_scales"] + torch.log1p(push)
    scene = types.SimpleNamespace(cameras=cams, train_indices=[1, 2, 3, 5, 6, 7], eval_indices=[0, 4])
    res = {}
    for name in variants:
        prior_on, smooth_on = VARIANTS[name]
        model = gs.SplatfactoDeblurModel.from_scene(cfg, start, dev)
        torch.manual_seed(0)
        r = T.train_scene(model, scene, images, steps, seed=3, normals=normals if prior_on else None,
                          normal_lambda=normal_lambda if prior_on else 0.0,
                          normal_smooth_lambda=smooth_lambda if smooth_on else 0.0, normal_edge_beta=edge_beta)
        res[name] = (held_out_angle(model, cams, normals, scene.eval_indices),
                     held_out_depth_l1(model, cams, depths, scene.eval_indices), r["results"]["psnr"])
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--normal-lambda", type=float, default=0.02)
    ap.add_argument("--normal-smooth-lambda", type=float, default=0.01)
    ap.add_argument("--normal-edge-beta", type=float, default=0.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "normal_train.jsonl"))
    args = ap.parse_args()
    import torch
    import gsdeblur_amd as gs
    dev = torch.device("cuda:0")
    t0 = time.time()
    res = run(gs, dev, args.steps, args.normal_lambda, args.normal_smooth_lambda, args.normal_edge_beta,
              variants=tuple(VARIANTS))
    line = {"tool": "normal_e2e", "scene": "3000 Gaussians, 128x96, 8 views (6 train, 2 held out), means pushed along the rays",
            "steps": args.steps, "normal_lambda": args.normal_lambda, "normal_smooth_lambda": args.normal_smooth_lambda,
            "normal_edge_beta": args.normal_edge_beta}
    for name, (angle, l1, psnr) in res.items():
        line[f"held_out_angle_deg_{name}"] = round(angle, 3)
        line[f"angle_ratio_{name}"] = round(angle / res["none"][0], 4)
        line[f"held_out_depth_l1_{name}"] = round(l1, 4)
        line[f"held_out_psnr_{name}"] = round(psnr, 3)
    line["seconds"] = round(time.time() - t0, 1)
    print(json.dumps(line))
    with open(args.out, "at") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
