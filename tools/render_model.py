#!/usr/bin/env python
"""Render a saved model over a dataset's images: the counterpart of the reference's render_model.py (:162-259), which
starts from `--load-config`; here the model comes from a checkpoint (gs.checkpoint.save_checkpoint, what
tools/train_deblur.py leaves as checkpoint_<name>.pt) or from a Gaussian-splat PLY.

  python tools/render_model.py --checkpoint out/checkpoint_blur_samples_5.pt --data /tmp/ds --set eval --out renders
  python tools/render_model.py --ply out/splat_blur_samples_5.ply --data /tmp/ds --out renders

For every image of the set: camera.metadata["cam_idx"] is set to the image's index (it selects the pose / velocity
adjustment a checkpoint carries), model.get_outputs_for_camera renders it, and <stem>_pred.png, <stem>_gt.png and
pred/depth/raw/<stem>.npy are written (the reference's names, render_model.py:101-104, 127-133).  metrics.json holds
{"results": {"psnr", "ssim"}} with training.evaluate's formulas; --color-correct adds <stem>_cc.png (the render after
gs.color_correct fitted its colours to the image) and cc_psnr / cc_ssim.  A PLY carries no camera-side parameters and no
training config: it renders with the defaults at the file's SH degree and --blur-samples (default 0: one sharp render).
--normals also writes the normals of the sharp render's depth (model.render_normals): <stem>_normal.png, the usual
picture (n * (1, -1, -1) + 1) / 2 with pixels without a normal black, and normal/<stem>.npy, the camera-frame vectors."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gsdeblur_amd as gs  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint", default=None)
    src.add_argument("--ply", default=None)
    ap.add_argument("--data", required=True, help="dataset root (transforms.json)")
    ap.add_argument("--set", default="eval", choices=["eval", "train"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--blur-samples", type=int, default=0, help="--ply only: blur samples of the render")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--color-correct", action="store_true",
                    help="also write <stem>_cc.png, the render fitted to its image by gs.color_correct, and cc_psnr / "
                         "cc_ssim into metrics.json")
    ap.add_argument("--normals", action="store_true",
                    help="also write <stem>_normal.png and normal/<stem>.npy: the normals of the sharp render's depth")
    ap.add_argument("--normal-min-alpha", type=float, default=0.5,
                    help="--normals: pixels whose accumulation is not above it have no depth, hence no normal")
    return ap


def normal_picture(normals):
    """[H,W,3] camera-frame normals -> the usual picture: (n * (1, -1, -1) + 1) / 2, pixels without a normal black"""
    has = (normals != 0).any(dim=-1, keepdim=True)
    return torch.where(has, (normals * normals.new_tensor([1.0, -1.0, -1.0]) + 1.0) * 0.5, torch.zeros_like(normals))


def main():
    args = build_parser().parse_args()
    dev = torch.device(args.device)
    scene = gs.load_transforms(args.data)
    images = gs.data.load_scene_images(scene, dev)
    if args.checkpoint:
        model = gs.checkpoint.load_checkpoint(args.checkpoint, dev).model
    else:
        sh_degree = gs.checkpoint.load_ply(args.ply)["sh_degree"]
        cfg = gs.SplatfactoDeblurConfig(sh_degree=sh_degree, blur_samples=args.blur_samples,
                                        gamma=2.2 if args.blur_samples > 0 else 1.0)
        model = gs.SplatfactoDeblurModel.from_ply(args.ply, cfg, dev, num_cameras=len(scene.cameras))
    indices = scene.eval_indices if args.set == "eval" else scene.train_indices
    os.makedirs(os.path.join(args.out, "pred", "depth", "raw"), exist_ok=True)
    if args.normals:
        os.makedirs(os.path.join(args.out, "normal"), exist_ok=True)
    ps, ss, cps, css = [], [], [], []
    for i in indices:
        camera = scene.cameras[i]
        camera.metadata["cam_idx"] = i
        out = model.get_outputs_for_camera(camera)
        rgb, depth = out["rgb"], out["depth"]
        stem = Path(scene.image_paths[i]).stem
        gs.data.save_image(os.path.join(args.out, f"{stem}_pred.png"), rgb)
        gs.data.save_image(os.path.join(args.out, f"{stem}_gt.png"), images[i])
        np.save(os.path.join(args.out, "pred", "depth", "raw", f"{stem}.npy"), depth.detach().cpu().numpy())
        if args.normals:
            normals = model.render_normals(camera, min_alpha=args.normal_min_alpha)
            gs.data.save_image(os.path.join(args.out, f"{stem}_normal.png"), normal_picture(normals))
            np.save(os.path.join(args.out, "normal", f"{stem}.npy"), normals.cpu().numpy())
        ps.append(gs.training.psnr(rgb, images[i]))
        ss.append(float(gs.training.ssim(rgb.clamp(0, 1), images[i]).item()))
        if args.color_correct:
            cc = gs.color_correct(rgb.clamp(0, 1), images[i])
            gs.data.save_image(os.path.join(args.out, f"{stem}_cc.png"), cc)
            cps.append(gs.training.psnr(cc, images[i]))
            css.append(float(gs.training.ssim(cc, images[i]).item()))
    results = {"psnr": sum(ps) / max(1, len(ps)), "ssim": sum(ss) / max(1, len(ss))}
    if args.color_correct:
        results.update(cc_psnr=sum(cps) / max(1, len(cps)), cc_ssim=sum(css) / max(1, len(css)))
    with open(os.path.join(args.out, "metrics.json"), "wt") as f:
        json.dump({"results": results, "set": args.set, "images": len(indices)}, f)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
