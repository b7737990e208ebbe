"""csrc/colorcorrect.hip on the GPU against the float64 reference (tests/colorcorrect_reference.py).

Bound (colorcorrect_reference.check_case; measured and printed, not chosen): 4 x max |reference(store=float32) -
reference(store=None)| on the same inputs + 1e-6 for the image; the same rule relative to max |w| for the warps.  A mask
decision that flips changes every pixel of a small image, so the cases up to 64 x 48 (and the one-row cases around the
kernel's pixel tile) have no pixel within 1e-6 of a threshold; at 480 x 270 at most 0.01 % of the pixels are (both
asserted; the seeds were chosen on the CPU).  Determinism is checked at 1920 x 1080, where no CPU reference is computed."""
import re
from pathlib import Path

import pytest
import torch

import colorcorrect_reference as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE = int(re.search(r"constexpr int kTile = (\d+);",
                     (ROOT / "3dgs-deblur_amd" / "csrc" / "colorcorrect.hip").read_text()).group(1))
ROWS = [(TILE - 1, 1), (TILE, 1), (TILE + 1, 1)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", R.SIZES + ROWS)
def test_kernels_against_the_reference(gs, dev, size, B):
    W, H = size
    k = R.case(B, H, W)
    out, warps = gs.color_correct(k["img"].to(dev), k["ref"].to(dev), return_warps=True)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (B, H, W, 3)
    assert warps.dtype == torch.float64 and warps.shape == (B, 5, 3, 10)
    R.check_case(k, out, warps, f"hip {W}x{H} B={B}")
    if B == 3:                                      # the single-image form, and independence of the batch
        one, w1 = gs.color_correct(k["img"][1].to(dev), k["ref"][1].to(dev), return_warps=True)
        assert one.shape == (H, W, 3) and torch.equal(one, out[1]) and torch.equal(w1, warps[1])


def test_two_runs_and_any_batch_agree_bit_for_bit_at_1080p(gs, dev):
    img, ref = (t.to(dev) for t in R.random_case(3, 1080, 1920, 77))
    a, wa = gs.color_correct(img, ref, return_warps=True)
    b, wb = gs.color_correct(img, ref, return_warps=True)
    assert torch.equal(a, b) and torch.equal(wa, wb)
    for i in (0, 2):
        one, w1 = gs.color_correct(img[i], ref[i], return_warps=True)
        assert torch.equal(one, a[i]) and torch.equal(w1, wa[i])
    assert torch.isfinite(a).all() and float((a - ref).abs().mean()) < float((img - ref).abs().mean())


def test_degenerate_inputs_keep_the_identity_warp(gs, dev):
    ref = R.random_case(1, 12, 16, 4)[1][0].to(dev)
    ident = gs.colorcorrect.identity_warps(1, 5, dev)[0]
    black = torch.zeros(12, 16, 3, device=dev)
    out, warps = gs.color_correct(black, ref, return_warps=True)
    assert torch.equal(out, black) and torch.equal(warps, ident)
    const = torch.full((12, 16, 3), 0.5, device=dev)
    out, warps = gs.color_correct(const, ref, return_warps=True)
    assert torch.isfinite(out).all() and torch.equal(out, const) and torch.equal(warps, ident)
    px, tgt = torch.full((1, 1, 3), 0.25, device=dev), torch.full((1, 1, 3), 0.75, device=dev)
    out, warps = gs.color_correct(px, tgt, return_warps=True)
    assert torch.equal(out, px) and torch.equal(warps, ident)
    img = R.random_case(1, 12, 16, 5)[0][0].to(dev)
    img[..., 1] = 0.5                               # one constant channel: rank-deficient for every output channel
    out, warps = gs.color_correct(img, ref, return_warps=True)
    assert torch.equal(out, img) and torch.equal(warps, ident)
    assert torch.equal(gs.color_correct(img, ref, num_iters=0), img)


def test_argument_checks(gs, dev):
    img, ref = (t[0].to(dev) for t in R.random_case(1, 5, 7, 6))
    with pytest.raises(ValueError):
        gs.color_correct(img, ref.cpu())
    with pytest.raises(ValueError):
        gs.color_correct(img, ref[:4])
    with pytest.raises(ValueError):
        gs.color_correct(img.double(), ref.double())
    out = gs.color_correct(img.clone().requires_grad_(True), ref)
    assert not out.requires_grad
    # a non-contiguous view is taken as it reads
    wide = torch.rand(5, 7, 6, device=dev) * 0.8 + 0.1
    assert torch.equal(gs.color_correct(wide[..., :3], ref), gs.color_correct(wide[..., :3].contiguous(), ref))


H_, W_ = 32, 48


def test_evaluate_on_the_gpu_agrees_with_the_cpu_fit_of_the_same_renders(gs, dev):
    """a small real scene, three cameras; ground truth = the render through an affine colour change plus noise.  The CPU
    side is the float32-stored reference on the SAME renders, PSNR by the same formula.  The image bound e of
    check_case (4 x the reference-only term + 1e-6, measured on these renders) is carried through PSNR = -10 log10(mse):
    an image error of at most e moves the mse by at most 2 e sqrt(mse) + e^2, the PSNR by at most
    10 / ln 10 * (2 e / sqrt(mse) + e^2 / mse); float32 evaluation of the mse itself adds 1e-6 relative."""
    import math
    sc = gs.data.synthetic_scene(1000, W_, H_, sh_degree=3, seed=12)
    # a mid-grey background ("auto" starts at sigmoid(0)): on black, most of a dark render sits near the lower threshold
    cfg = gs.SplatfactoDeblurConfig(blur_samples=2, rolling_shutter_compensation=False, background_color="auto")
    model = gs.SplatfactoDeblurModel.from_scene(cfg, sc, dev, num_cameras=3)
    flip = torch.tensor([1.0, -1.0, -1.0])
    cams = []
    for i in range(3):
        c2w = torch.eye(4)[:3].clone()
        c2w[:, 1] *= -1
        c2w[:, 2] *= -1
        c2w[0, 3] = 0.05 * (i - 1)
        cams.append(gs.Camera(c2w, sc["fx"], sc["fy"], sc["cx"], sc["cy"], W_, H_,
                              metadata=dict(cam_idx=i, camera_linear_velocity=[float(v) for v in sc["lin_vel"] * flip],
                                            camera_angular_velocity=[float(v) for v in sc["ang_vel"] * flip],
                                            exposure_time=1 / 60, rolling_shutter_time=0.0)))
    renders = [model.get_outputs_for_camera(c)["rgb"].clamp(0, 1) for c in cams]
    assert float(torch.stack(renders).std()) > 0.02                      # something was rendered
    noise = torch.rand(H_, W_, 3, generator=torch.Generator().manual_seed(8)).to(dev) - 0.5
    gain, offset = torch.tensor([0.8, 0.9, 0.85], device=dev), torch.tensor([0.04, 0.03, 0.05], device=dev)
    images = [(r * gain + offset + 0.02 * noise).clamp(0, 1) for r in renders]
    plain = gs.training.evaluate(model, cams, images, [0, 1, 2])
    assert set(plain) == {"psnr", "ssim"}
    on = gs.training.evaluate(model, cams, images, [0, 1, 2], color_corrected=True)
    batched = gs.training.evaluate(model, cams, images, [0, 1, 2], batch_size=3, color_corrected=True)
    assert set(on) == {"psnr", "ssim", "cc_psnr", "cc_ssim"} and on["psnr"] == plain["psnr"]
    assert batched["cc_psnr"] == on["cc_psnr"] and batched["cc_ssim"] == on["cc_ssim"]
    want, tol = 0.0, 0.0
    for r, im in zip(renders, images):
        r, im = r.cpu(), im.cpu()
        out32, out64 = R.reference(r, im)[0], R.reference(r, im, store=None)[0]
        assert int(R.fragile(r, im).sum()) == 0           # a flipped mask decision moves every pixel of so small an image
        e = 4.0 * float((out32 - out64).abs().max()) + 1e-6
        mse = float(((out32 - im.double()) ** 2).mean())
        want += gs.training.psnr(out32.float(), im) / 3
        tol += 10.0 / math.log(10.0) * (2 * e / math.sqrt(mse) + e * e / mse + 1e-6) / 3
    print(f"psnr {on['psnr']:.3f}, cc_psnr gpu {on['cc_psnr']:.6f} reference {want:.6f}, tolerance {tol:.2e}")
    assert abs(on["cc_psnr"] - want) <= tol
    assert on["cc_psnr"] > on["psnr"]
