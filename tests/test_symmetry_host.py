"""The float64 oracle under the three exact symmetries of symmetry_cases.py, at general intrinsics (fx != fy, the
principal point off the centre) and a non-identity pose, for six sub-pose structures.  No GPU.

A scene variant X(scene) must render X(image), flag X(fragile mask), and its gradients must map back to the scene's own:
image within 1e-12 absolute, gradients within 1e-11 of the tensor's maximum (measured: 7e-16 and 4.2e-15; the margin
covers another summation order and is far below any fp32 effect).  If the oracle violated a relation, its restatement
would be wrong — and the GPU test (test_gpu_symmetry.py) could not tell a kernel's fault from the oracle's.
One negative control proves that the file can fail.
"""
import functools

import pytest
import torch

import gs_oracle as O
import symmetry_cases as SC

IMG_BAR = 1e-12
GRAD_BAR = 1e-11


@functools.lru_cache(maxsize=None)
def _base():
    return SC.base_scene(O)


def _frame(sc, cfg_kw, wt):
    """oracle frame + backward of sum(img * wt) + sum(alpha * wt[..., 0]) off the fragile pixels"""
    f = SC.oracle_forward(O, sc, cfg_kw)
    good = (~f["frag"]).double()
    ((f["img"] * wt * good[..., None]).sum() + (f["alpha"] * wt[..., 0] * good).sum()).backward()
    f["grads"] = SC.grads_of(f["q"])
    return f


@functools.lru_cache(maxsize=None)
def _identity_frame(name):
    return _frame(_base(), SC.HOST_CONFIGS[name], SC.loss_weights())


@pytest.mark.parametrize("name", list(SC.HOST_CONFIGS))
def test_fragile_share_is_under_the_cap_the_gpu_tests_rely_on(name):
    share = float(_identity_frame(name)["frag"].double().mean())
    print(f"[symmetry fragile {name}] {share:.5f}")
    assert share <= SC.FRAGILE_CAP, (name, share)


# (the transpose is not claimed with a rolling shutter: rows become columns)
@pytest.mark.parametrize("name,variant", [(n, v) for n, kw in SC.HOST_CONFIGS.items() for v in SC.variants_of(kw)[1:]])
def test_oracle_is_symmetric(name, variant):
    cfg_kw = SC.HOST_CONFIGS[name]
    ref = _identity_frame(name)
    f = _frame(SC.map_scene(variant, _base()), cfg_kw, SC.map_image(variant, SC.loss_weights()))
    assert torch.equal(SC.map_image(variant, f["frag"]), ref["frag"]), (name, variant)
    d_img = float((SC.map_image(variant, f["img"].detach()) - ref["img"].detach()).abs().max())
    d_alpha = float((SC.map_image(variant, f["alpha"].detach()) - ref["alpha"].detach()).abs().max())
    back = SC.map_params(variant, f["grads"])
    d_grad = {k: SC.rel_to_max(back[k], ref["grads"][k]) for k in SC.NAMES}
    print(f"[symmetry host {name} {variant}] image {d_img:.2e} alpha {d_alpha:.2e} gradients "
          + " ".join(f"{k} {v:.1e}" for k, v in d_grad.items()))
    assert d_img <= IMG_BAR and d_alpha <= IMG_BAR, (name, variant, d_img, d_alpha)
    for k, v in d_grad.items():
        assert float(ref["grads"][k].abs().max()) > 0, k        # a relation on a zero gradient would say nothing
        assert v <= GRAD_BAR, (name, variant, k, v)


def test_negative_control_transpose_without_permuted_scales_fails():
    """the file can fail: the transpose with the scale columns NOT permuted is no symmetry (measured residual 0.39)"""
    name = "se3 S=3"
    ref = _identity_frame(name)
    sc = SC.map_scene("transpose", _base())
    sc["log_scales"] = _base()["log_scales"]
    f = SC.oracle_forward(O, sc, SC.HOST_CONFIGS[name])
    d = float((SC.map_image("transpose", f["img"].detach()) - ref["img"].detach()).abs().max())
    print(f"[symmetry host negative control] transpose residual without the scale permutation {d:.3f}")
    assert d > 1e-3, d


def test_maps_are_involutions():
    sc = _base()
    for variant in SC.VARIANTS[1:]:
        twice = SC.map_scene(variant, SC.map_scene(variant, sc))
        for k in SC.NAMES:
            assert torch.equal(twice[k], sc[k]), (variant, k)
        for k in ("fx", "fy", "width", "height"):
            assert twice[k] == sc[k], (variant, k)
        for k in ("cx", "cy"):
            assert abs(twice[k] - sc[k]) < 1e-12, (variant, k)
