"""Reference-made fixture for the blur-scored evaluation split (data.split_indices(eval_mode="blur_score"),
data.write_blur_scored).

Runs in the BUILD CONTAINER only: it imports /root/reference/train_eval_split_by_blur_score.py at run time and calls its
`process` unmodified on temporary folders.  Only data travels, as tests/golden/ref_blur_split.json: per case the input
transforms.json, the transforms.json the reference wrote and the sorted list of the files it wrote.
tests/test_blur_host.py must reproduce both from the input.

Cases: 19 frames listed out of path order with interval 8 and tied scores inside a run (the reference takes the first of a
tie in path order: sorted() is stable); 16 frames with interval 4; 5 frames with interval 8 (one short run).
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, REF / (name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def input_transforms(n, seed, shuffle, ties):
    rng = np.random.default_rng(seed)
    scores = [round(float(s), 3) for s in rng.uniform(0.1, 2.0, n)]
    for run_start, a, b in ties:                     # the run's minimum, twice: frames a < b of that run
        low = min(scores[run_start:run_start + 8]) - 0.05
        scores[a] = scores[b] = round(low, 3)
    frames = []
    for i in range(n):
        m = np.eye(4)
        m[:3, 3] = rng.uniform(-1, 1, 3)
        frames.append({"file_path": "images/frame_%05d.png" % i, "transform_matrix": m.tolist(),
                       "camera_linear_velocity": rng.uniform(-1, 1, 3).tolist(),
                       "camera_angular_velocity": rng.uniform(-1, 1, 3).tolist(), "motion_blur_score": scores[i],
                       "colmap_im_id": i + 1})
    if shuffle:
        frames = [frames[i] for i in rng.permutation(n)]
    return {"w": 64, "h": 48, "fl_x": 60.0, "fl_y": 60.0, "cx": 32.0, "cy": 24.0, "k1": 0.0, "k2": 0.0, "p1": 0.0, "p2": 0.0,
            "exposure_time": 0.02, "rolling_shutter_time": 0.03, "aabb_scale": 16, "frames": frames}


def make():
    splitter = _load("train_eval_split_by_blur_score")
    out = {"source": "/root/reference/train_eval_split_by_blur_score.py::process (:6-57), called unmodified on a temporary "
                     "folder", "cases": []}
    for n, interval, seed, shuffle, ties in ((19, 8, 41, True, ((0, 2, 5), (8, 9, 15))), (16, 4, 42, False, ()),
                                             (5, 8, 43, False, ())):
        src = input_transforms(n, seed, shuffle, ties)
        with tempfile.TemporaryDirectory() as td:
            inp, prefix = os.path.join(td, "in", "scene"), os.path.join(td, "out")
            os.makedirs(os.path.join(inp, "images"))
            for fr in src["frames"]:
                with open(os.path.join(inp, fr["file_path"]), "wb") as f:
                    f.write(fr["file_path"].encode())
            with open(os.path.join(inp, "sparse_pc.ply"), "wt") as f:
                f.write("ply\n")
            with open(os.path.join(inp, "transforms.json"), "wt") as f:
                json.dump(src, f)
            splitter.process(inp, prefix, argparse.Namespace(interval=interval, dry_run=False))
            dst = os.path.join(prefix, "scene")
            with open(os.path.join(dst, "transforms.json")) as f:
                written = json.load(f)
            files = sorted(os.path.relpath(os.path.join(d, name), dst) for d, _, names in os.walk(dst) for name in names)
        out["cases"].append({"interval": interval, "input_transforms": src, "output_transforms": written, "files": files})
    return out


def main():
    if not REF.exists():
        sys.exit("needs /root/reference (build container only)")
    with open(HERE / "ref_blur_split.json", "wt") as f:
        json.dump(make(), f, indent=1)
    print("wrote", HERE / "ref_blur_split.json")


if __name__ == "__main__":
    main()
