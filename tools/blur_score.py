"""Score every frame of a dataset by how blurred the motion model predicts it to be, and cut the blur-scored
train / evaluation split the reference trains on (/root/reference/train_eval_split_by_blur_score.py) — without sai-cli.

The score of a frame is gs.blur_stats' mean_blur: the mean length in pixels of the streak its exposure draws, over the
points it sees.  Without --checkpoint it comes from the dataset alone — poses, camera_linear_velocity /
camera_angular_velocity, exposure_time — and the seed cloud (ply_file_path, or sparse_pc.ply beside transforms.json);
--from-poses replaces the stored velocities by finite differences of the poses (data.velocities_from_poses, for
pose-only datasets, in units of --fps).  With --checkpoint the trained model scores its own means with the poses,
velocities and times it learned (model.blur_scores): the reference's "2nd pass" — train once with zero-initialised
velocity optimisation, score, split, train again.

    python tools/blur_score.py --data ROOT --write-scores                 # motion_blur_score into ROOT/transforms.json
    python tools/blur_score.py --data ROOT --split-to DST [--interval 8]  # DST: eval_/train_ copies, --eval-mode filename
    python tools/blur_score.py --data ROOT --checkpoint CKPT --split-to DST

Runs on the GPU when there is one (the HIP kernels), else on the CPU (the torch form)."""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def seed_cloud(gs, scene, root: str):
    for path in (scene.ply_file_path, os.path.join(root, "sparse_pc.ply")):
        if path and os.path.exists(path):
            return gs.load_seed_points_ply(path)[0]
    raise SystemExit("no seed cloud: transforms.json names no ply_file_path and there is no sparse_pc.ply (use --checkpoint)")


def compute_scores(gs, args, device):
    import torch
    scene = gs.load_transforms(args.data, eval_mode="all")
    root = args.data if os.path.isdir(args.data) else os.path.dirname(args.data)
    if args.from_poses:
        c2w = torch.stack([c.camera_to_world[:3] for c in scene.cameras])
        lin, ang = gs.data.velocities_from_poses(c2w, times=[i / args.fps for i in range(len(scene.cameras))])
        for cam, l, a in zip(scene.cameras, lin.tolist(), ang.tolist()):
            cam.metadata["camera_linear_velocity"], cam.metadata["camera_angular_velocity"] = l, a
    if args.checkpoint:
        model = gs.checkpoint.load_checkpoint(args.checkpoint, device=device).model
        return scene, model.blur_scores(scene.cameras)
    return scene, gs.data.blur_scores(scene, seed_cloud(gs, scene, root).to(device))


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="dataset folder (or its transforms.json)")
    ap.add_argument("--checkpoint", default=None, help="score with a trained model instead of the dataset's metadata")
    ap.add_argument("--interval", type=int, default=8, help="frames per run; one evaluation frame is taken from each")
    ap.add_argument("--from-poses", action="store_true", help="finite-difference velocities instead of the stored ones")
    ap.add_argument("--fps", type=float, default=30.0, help="--from-poses: frames per second of the sequence")
    ap.add_argument("--device", default=None, help="cuda:0 when there is a GPU, else cpu")
    out = ap.add_mutually_exclusive_group(required=True)
    out.add_argument("--write-scores", action="store_true", help="store motion_blur_score in the dataset's transforms.json")
    out.add_argument("--split-to", default=None, metavar="DST", help="write the blur-scored copy of the dataset here")
    args = ap.parse_args(argv)

    import torch
    import gsdeblur_amd as gs
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    scene, scores = compute_scores(gs, args, device)
    root = args.data if os.path.isdir(args.data) else os.path.dirname(args.data)
    for path, s in zip(scene.image_paths, scores):
        print(f"{os.path.basename(path)} {s:.4f}")
    if args.split_to:
        print("wrote", gs.data.write_blur_scored(root, args.split_to, scores=scores, interval=args.interval))
        return
    json_path = os.path.join(root, "transforms.json")
    with open(json_path, "rt") as f:
        meta = json.load(f)
    by_path = {os.path.normpath(os.path.join(root, fr["file_path"])): fr for fr in meta["frames"]}
    for path, s in zip(scene.image_paths, scores):
        by_path[path]["motion_blur_score"] = float(s)
    tmp = json_path + ".tmp"
    with open(tmp, "wt") as f:
        json.dump(meta, f, indent=4)
    os.replace(tmp, json_path)
    print("wrote", json_path)


if __name__ == "__main__":
    main()
