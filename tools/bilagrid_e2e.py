"""End-to-end check of the bilateral-grid colour correction: the self-generated blurred dataset of tools/densify_e2e.py
with every TRAINING image multiplied by a seeded per-image, per-channel gain (what auto-exposure and auto-white-balance
do to handheld video); the evaluation images are left untouched.  Trained with and without the grid, and once on the
unperturbed images for scale.  Sharp-frame PSNR / SSIM of the UNCORRECTED evaluation renders, the same two metrics after
the colour fit of gs.color_correct (cc_psnr / cc_ssim; evaluation happens after the clock stops) and the training seconds.
One scene, one seed.
usage: python tools/bilagrid_e2e.py [iterations] [--record]   (--record appends the result to profiles/bilagrid_train.jsonl)"""
import json
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gsdeblur_amd as gs          # noqa: E402
import synthetic_dataset as SD     # noqa: E402

record = "--record" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--record"]
iters = int(argv[0]) if argv else 2000
GAIN_SPREAD = 0.2                  # gains uniform in [1 - 0.2, 1 + 0.2], per image and channel
dev = torch.device("cuda", 0)
root = tempfile.mkdtemp()
SD.generate(root, dev, width=240, height=160, n_frames=24, n_gaussians=8000, speed=1.0, dense_samples=32, seed_points=1500)
scene = gs.load_transforms(root)
clean = gs.data.load_scene_images(scene, dev)
xyz, rgb = gs.load_seed_points_ply(scene.ply_file_path)
g = torch.Generator().manual_seed(17)
gains = 1.0 + GAIN_SPREAD * (2.0 * torch.rand(len(clean), 3, generator=g) - 1.0)
train = set(scene.train_indices) - set(scene.eval_indices)
perturbed = [(img * gains[i].to(dev)).clamp(0, 1) if i in train else img for i, img in enumerate(clean)]
res = {}
for name, images, grid in (("clean_images", clean, False), ("gains_no_grid", perturbed, False),
                           ("gains_with_grid", perturbed, True)):
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0,
                                    rolling_shutter_compensation=False, use_scale_regularization=True,
                                    use_bilateral_grid=grid, color_corrected_metrics=True)
    model = SD.init_from_seed_points(cfg, xyz, rgb, dev, num_cameras=len(scene.cameras))
    r = gs.training.train_scene(model, scene, images, iters)
    res[name] = {"psnr": round(r["results"]["psnr"], 3), "ssim": round(r["results"]["ssim"], 4),
                 "cc_psnr": round(r["results"]["cc_psnr"], 3), "cc_ssim": round(r["results"]["cc_ssim"], 4),
                 "seconds": round(r["wall_clock_time_seconds"], 2)}
    if grid:
        dev_from_identity = (model.bilateral_grids.detach() - gs.bilagrid.identity_grids(1).to(dev)).abs().flatten(1).max(1)[0]
        res[name]["grids_moved"] = int((dev_from_identity > 1e-3).sum())
    print(name, json.dumps(res[name]), flush=True)
line = json.dumps({"iterations": iters, "gain_spread": GAIN_SPREAD, "train_images": len(train),
                   "eval_images": len(scene.eval_indices), "results": res})
print(line)
if record:
    with open(ROOT / "profiles" / "bilagrid_train.jsonl", "a") as fh:
        fh.write(line + "\n")
