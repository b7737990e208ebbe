#!/usr/bin/env python
"""Export a triangle mesh of a saved model: the counterpart of nerfstudio's `ns-export tsdf`.  The model comes from a
checkpoint (gs.checkpoint.save_checkpoint, what tools/train_deblur.py leaves as checkpoint_<name>.pt) or from a
Gaussian-splat PLY, the views from a dataset's cameras.

  python tools/export_mesh.py --checkpoint out/checkpoint_blur_samples_5.pt --data /tmp/ds --set train --out mesh.ply
  python tools/export_mesh.py --ply out/splat_blur_samples_5.ply --data /tmp/ds --set all --resolution 512 --out mesh.ply

Every camera of the set is rendered sharp (exposure and readout 0 at its effective pose; camera.metadata["cam_idx"] is
set to the image's index so that a checkpoint's pose adjustment applies), depth and colour are fused into a TSDF volume
(model.fuse_tsdf: the box of the means between the 2nd and 98th percentile, --resolution samples along its longest
axis, truncation 4 voxels, pixels with accumulation below --min-alpha left out), and the zero level set is written as a
binary PLY with vertex colours (gs.tsdf.write_mesh_ply).  --keep-largest K and --min-component-faces N remove small
connected components first (gs.mesh_filter_components: the floaters of a splat model); both are off by default and the
file is then what it was without them.  --decimate-cell S and --target-faces N then decimate the mesh by vertex
clustering (gs.mesh_decimate): at cell size S, or at the first size of the ladder above the volume's voxel size (above S
when both are given) that leaves at most N faces; both off: nothing runs.  The order is extract, clean, decimate:

  python tools/export_mesh.py --checkpoint ck.pt --data /tmp/ds --out mesh.ply --keep-largest 1 --target-faces 100000

Prints one JSON line: vertices, faces, volume dims, seconds, with a clean-up option on the components found and kept, and
with a decimation option on the cell size used, the clusters and the faces before decimation."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gsdeblur_amd as gs  # noqa: E402


def clean_mesh(verts, faces, colors, keep_largest=None, min_component_faces=None):
    """-> (verts, faces, colors, what the JSON line gains): the mesh itself, untouched, with both options off"""
    if keep_largest is None and min_component_faces is None:
        return verts, faces, colors, {}
    verts, faces, colors, stats = gs.mesh_filter_components(verts, faces, colors, min_faces=min_component_faces or 1,
                                                            keep_largest=keep_largest, return_stats=True)
    return verts, faces, colors, {"components": stats["components"], "kept": stats["kept"]}


def decimate_mesh(verts, faces, colors, voxel_size, decimate_cell=None, target_faces=None):
    """-> (verts, faces, colors, what the JSON line gains): the mesh itself, untouched, with both options off"""
    if decimate_cell is None and target_faces is None:
        return verts, faces, colors, {}
    verts, faces, colors, stats = gs.mesh_decimate(verts, faces, colors, cell_size=voxel_size if decimate_cell is None else decimate_cell,
                                                   target_faces=target_faces, return_stats=True)
    return verts, faces, colors, {"decimate_cell": stats["cell_size"], "clusters": stats["clusters"],
                                  "faces_before_decimation": stats["faces_in"]}


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint", default=None)
    src.add_argument("--ply", default=None)
    ap.add_argument("--data", required=True, help="dataset root (transforms.json)")
    ap.add_argument("--set", default="train", choices=["train", "eval", "all"])
    ap.add_argument("--resolution", type=int, default=256, help="samples along the longest axis of the volume")
    ap.add_argument("--out", required=True)
    ap.add_argument("--min-alpha", type=float, default=0.5)
    ap.add_argument("--depth-max", type=float, default=None)
    ap.add_argument("--min-weight", type=float, default=0.0, help="use only cells whose corners were seen more than this")
    ap.add_argument("--keep-largest", type=int, default=None, help="keep only the K connected components with the most faces")
    ap.add_argument("--min-component-faces", type=int, default=None, help="drop connected components with fewer faces")
    ap.add_argument("--decimate-cell", type=float, default=None, help="decimate by vertex clustering at this cell size")
    ap.add_argument("--target-faces", type=int, default=None,
                    help="decimate to at most this many faces (cell sizes from the voxel size, or --decimate-cell, upwards)")
    ap.add_argument("--blurred", action="store_true", help="fuse the renders as the model blurs them (default: sharp)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    dev = torch.device(args.device)
    scene = gs.load_transforms(args.data)
    if args.checkpoint:
        model = gs.checkpoint.load_checkpoint(args.checkpoint, dev).model
    else:
        sh_degree = gs.checkpoint.load_ply(args.ply)["sh_degree"]
        model = gs.SplatfactoDeblurModel.from_ply(args.ply, gs.SplatfactoDeblurConfig(sh_degree=sh_degree), dev,
                                                  num_cameras=len(scene.cameras))
    indices = {"train": scene.train_indices, "eval": scene.eval_indices,
               "all": sorted(set(scene.train_indices) | set(scene.eval_indices))}[args.set]
    cameras = []
    for i in indices:
        scene.cameras[i].metadata["cam_idx"] = i
        cameras.append(scene.cameras[i])
    t0 = time.time()
    volume = model.fuse_tsdf(cameras, resolution=args.resolution, min_alpha=args.min_alpha, depth_max=args.depth_max,
                             sharp=not args.blurred)
    verts, faces, colors = gs.tsdf_extract_mesh(volume, min_weight=args.min_weight)
    verts, faces, colors, cleaned = clean_mesh(verts, faces, colors, args.keep_largest, args.min_component_faces)
    verts, faces, colors, decimated = decimate_mesh(verts, faces, colors, volume.voxel_size, args.decimate_cell,
                                                    args.target_faces)
    gs.tsdf.write_mesh_ply(args.out, verts, faces, colors)
    print(json.dumps({"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "dims": list(volume.dims),
                      "voxel_size": volume.voxel_size, "views": len(cameras), "seconds": round(time.time() - t0, 3),
                      **cleaned, **decimated}))


if __name__ == "__main__":
    main()
