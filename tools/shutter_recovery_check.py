"""End-to-end check of the camera-shutter optimizer (SplatfactoDeblurConfig.camera_shutter_optimizer): ground-truth
Gaussians, frames rendered with rolling shutter AND motion blur from the true velocities at KNOWN exposure and readout
times (per-pixel-row ground truth, tools/synthetic_dataset.render_rolling_shutter_frame — none of the renderer's own
schedule), cameras whose metadata holds WRONG times, and a model that learns one global log-scale adjustment per time
through the gradient of the sub-pose times (gs_subpose_viewmats_bwd_times), Gaussians constant.  Prints, per start, the
learned / true ratio of each time and the loss of every frame before and after.

    python tools/shutter_recovery_check.py [--lr 1e-3 2e-3 5e-3 1e-2] [--iterations 150] [--frames 4]

recover() is what tests/test_gpu_shutter.py runs; the sweep over --lr is how training.SHUTTER_LR was chosen."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import gsdeblur_amd as gs          # noqa: E402
import synthetic_dataset as SD     # noqa: E402
from gsdeblur_amd.model import Camera   # noqa: E402

H, W = 120, 160
EXPOSURE = READOUT = 1 / 15
STARTS = {"exposure": ((0.5, 1.0), (2.0, 1.0)), "readout": ((1.0, 0.5), (1.0, 2.0)), "joint": ((0.5, 2.0), (2.0, 0.5))}


def ground_truth(dev, n_frames: int = 4):
    """(gt scene, trajectory, frame ids, {id: target image}): the moving frames of the velocity-recovery check"""
    gt = SD.make_gt_scene(4000, 0)
    traj = SD.trajectory(17, 1.5, 0)
    frames = [i for i in range(len(traj)) if i % 8 != 0][:n_frames]
    ref_cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=1, gamma=2.2, min_rgb_level=0.0, background_color="black",
                                        rolling_shutter_compensation=False)
    ref_model = gs.SplatfactoDeblurModel.from_scene(ref_cfg, gt, dev).eval()
    imgs = {}
    with torch.no_grad():
        for i in frames:
            imgs[i] = SD.render_rolling_shutter_frame(ref_model, _camera(traj, i, EXPOSURE, READOUT), EXPOSURE, READOUT, 2.2)
    return gt, traj, frames, imgs


def _camera(traj, i, exposure, readout):
    fr = traj[i]
    md = dict(cam_idx=i, camera_linear_velocity=fr["lin"].tolist(), camera_angular_velocity=fr["ang"].tolist(),
              exposure_time=exposure, rolling_shutter_time=readout)
    return Camera(fr["c2w"][:3], 0.75 * W, 0.75 * W, W / 2.0, H / 2.0, W, H, metadata=md)


def shutter_step(model, opt, camera, image) -> float:
    """one step in which only the shutter adjustments move: the Gaussians are constants (detach_gaussians)"""
    opt.zero_grad(set_to_none=True)
    out = model.get_outputs(camera, detach_gaussians=True)
    loss = gs.training.image_loss(out["rgb"], image)
    loss.backward()
    gs.training.optimizers_step([opt])
    return float(loss.item())


def recover(dev, truth, which: str, e_mult: float, r_mult: float, iterations: int, lr=None):
    """metadata times = (e_mult, r_mult) x the true ones; learn a global adjustment for `which` ("exposure", "readout"
    or "joint") over `iterations` passes through the frames.
    -> {"exposure_ratio", "readout_ratio" (learned / true), "first", "last" ({frame: loss}), "gauss_grads"}"""
    gt, traj, frames, imgs = truth
    cfg = gs.SplatfactoDeblurConfig(sh_degree=3, blur_samples=5, gamma=2.2, min_rgb_level=0.0, background_color="black",
                                    rolling_shutter_compensation=True, rs_bands=8)
    cfg.camera_shutter_optimizer.exposure = "global" if which in ("exposure", "joint") else "off"
    cfg.camera_shutter_optimizer.readout = "global" if which in ("readout", "joint") else "off"
    model = gs.SplatfactoDeblurModel.from_scene(cfg, gt, dev, num_cameras=len(traj))
    model.train()
    opt = gs.training.make_optimizers(model)["camera_shutter_opt"]
    if lr is not None:
        opt.param_groups[0]["lr"] = float(lr)
    cams = {i: _camera(traj, i, e_mult * EXPOSURE, r_mult * READOUT) for i in frames}
    first = {}
    for _ in range(iterations):
        for i in frames:
            loss = shutter_step(model, opt, cams[i], imgs[i])
            first.setdefault(i, loss)
    with torch.no_grad():
        last = {i: float(gs.training.image_loss(model.get_outputs(cams[i], detach_gaussians=True)["rgb"], imgs[i]).item())
                for i in frames}
        E, T = model.shutter_times(cams[frames[0]])
    return {"exposure_ratio": float(E) / EXPOSURE, "readout_ratio": float(T) / READOUT, "first": first, "last": last,
            "gauss_grads": [k for k, v in model.gauss_params().items() if v.grad is not None]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lr", type=float, nargs="+", default=[gs.training.SHUTTER_LR])
    ap.add_argument("--iterations", type=int, default=150, help="passes through the frames per start")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=None, help="append one JSON line per (lr, run, start) here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    truth = ground_truth(dev, args.frames)
    bound = 0.5 * math.log(2.0)
    for lr in args.lr:
        met = True
        for which, starts in STARTS.items():
            for e_mult, r_mult in starts:
                r = recover(dev, truth, which, e_mult, r_mult, args.iterations, lr)
                errs = {k: abs(math.log(r[k + "_ratio"])) for k, m in (("exposure", e_mult), ("readout", r_mult)) if m != 1.0}
                ok = all(v < bound for v in errs.values()) and all(r["last"][i] < r["first"][i] for i in r["first"])
                met = met and ok
                print(f"lr {lr:g} {which:8s} start E x{e_mult:g} T x{r_mult:g}: learned/true E {r['exposure_ratio']:.3f} "
                      f"T {r['readout_ratio']:.3f}   loss " +
                      " ".join(f"{r['first'][i]:.4f}->{r['last'][i]:.4f}" for i in r["first"]) + ("   ok" if ok else "   MISSED"),
                      flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps({"lr": lr, "run": which, "start": [e_mult, r_mult], "iterations": args.iterations,
                                             "frames": args.frames, "exposure_ratio": r["exposure_ratio"],
                                             "readout_ratio": r["readout_ratio"], "ok": ok}) + "\n")
        print(f"lr {lr:g}: recovery condition |ln(learned/true)| < ln(2)/2 and falling losses "
              f"{'met' if met else 'NOT met'} from every start", flush=True)


if __name__ == "__main__":
    main()
