"""Pooled gradient buffers (ops._grad_pool, gs_project_fused_bwd_pooled): a step that recycles the buffer of an earlier
step — only its dirty rows zeroed, touched flags cleared by their last reader — must give bit for bit the gradients of
the same frame rendered with pooling off (fresh buffers, full zero fill), whatever the caller did with the earlier
gradients.  N = 5000 = two full chunks of the sparse projection backward (2048 Gaussians a block) and a partial one."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

N, W, H, S = 5000, 96, 80, 2
GAUSS = ("means", "scales", "quats", "opacities", "sh", "sh_rest")
CAMERA = ("viewmat", "lin_vel", "ang_vel")


def _rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    V = torch.eye(4)
    V[0, 0], V[0, 2], V[2, 0], V[2, 2] = c, s, -s, c
    return V


class Scene:
    """parameters on the device + the two cameras; variant: 'deg3' | 'split' (features_dc / features_rest) | 'deg1'"""

    def __init__(self, gs, oracle, dev, variant, n=N, seed=7, sc=None):
        self.gs, self.dev, self.variant = gs, dev, variant
        self.deg = 1 if variant == "deg1" else 3
        sc = sc or oracle.synthetic_scene(n, W, H, sh_degree=self.deg, seed=seed, scale_mult=8.0)
        self.sc = sc
        self.p = {k: sc[k].float().to(dev).contiguous() for k in
                  ("means", "log_scales", "quats", "opacity_logits", "sh", "lin_vel", "ang_vel")}
        self.p["lin_vel"], self.p["ang_vel"] = self.p["lin_vel"] * 20, self.p["ang_vel"] * 10
        times, _, _ = gs.subpose_schedule(S, 1 / 60, 1, 0.0)
        self.times = torch.tensor(times, device=dev)
        self.wt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(3)).to(dev)
        self.cams = {"A": torch.eye(4).to(dev), "B": _rot_y(28.0).to(dev), "A2": _rot_y(0.6).to(dev)}
        self.n = self.p["means"].shape[0]

    def sh_args(self):
        if self.variant == "split":
            return self.p["sh"][:, 0].contiguous(), self.p["sh"][:, 1:].contiguous()
        return self.p["sh"], None

    def step(self, cam, hints=None, first=None):
        """one gs.render_step -> the gradients, as the caller gets them (views of the pooled buffer)"""
        sc, p = self.sc, self.p
        sh, sh_rest = self.sh_args()
        sl = slice(None) if first is None else slice(0, first)
        _, g, _ = self.gs.render_step(p["means"][sl], p["log_scales"][sl], p["quats"][sl], p["opacity_logits"][sl], sh[sl],
                                      self.cams[cam], p["lin_vel"], p["ang_vel"], self.times, None, S, 1, sc["fx"],
                                      sc["fy"], sc["cx"], sc["cy"], H, W, self.wt, gamma=2.2, min_rgb_level=10.0,
                                      sh_degree=self.deg, sh_rest=None if sh_rest is None else sh_rest[sl], hints=hints)
        return {k: v for k, v in g.items() if v is not None}

    def reference(self, cam, first=None):
        """the same frame with pooling off (fresh buffers, the kernel's full zero fill), copied out"""
        from gsdeblur_amd import ops
        ops.GRAD_POOL = False
        try:
            return {k: v.clone() for k, v in self.step(cam, first=first).items()}
        finally:
            ops.GRAD_POOL = True


_scenes = {}


def scene(gs, oracle, dev, variant):
    """one scene and ONE pooled-off reference per (variant, camera), shared by the tests and never written to"""
    if variant not in _scenes:
        s = Scene(gs, oracle, dev, variant)
        _scenes[variant] = (s, {c: s.reference(c) for c in ("A", "B")})
    return _scenes[variant]


@pytest.fixture()
def ops(gs):
    from gsdeblur_amd import ops
    ops.release_arenas()
    assert ops.GRAD_POOL
    yield ops
    ops.release_arenas()


def entries(ops):
    return [e for es in ops._grad_pool.values() for e in es]


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)


def touched_rows(g):
    n = g["means"].shape[0]
    return torch.stack([(g[k].reshape(n, -1) != 0).any(1) for k in GAUSS if k in g]).any(0)


def check_pool_state(ops, g):
    """after a step: the persistent touched flags are all zero again, and the dirty map covers every row written"""
    live = [e for e in entries(ops) if e.flat.data_ptr() == g["means"].data_ptr()]
    assert len(live) == 1
    e = live[0]
    assert e.valid and int(e.touched.count_nonzero()) == 0
    assert bool((e.dirty.bool() | ~touched_rows(g)).all())
    return e


@pytest.mark.parametrize("variant", ["deg3", "split", "deg1"])
def test_a_b_a_through_one_pool_equals_the_unpooled_frames(gs, oracle, dev, ops, variant):
    s, ref = scene(gs, oracle, dev, variant)
    only_a = touched_rows(ref["A"]) & ~touched_rows(ref["B"])
    only_b = touched_rows(ref["B"]) & ~touched_rows(ref["A"])
    assert int(only_a.sum()) > 20 and int(only_b.sum()) > 20             # camera B reaches other rows than A
    hints = ops.FrameHints()
    ptrs = []
    for i, cam in enumerate("ABA"):
        g = s.step(cam, hints)
        same(g, ref[cam], (variant, i, cam))
        if cam == "B":
            for k in GAUSS:
                if k in g:
                    assert not g[k][only_a].any(), (variant, k)                  # what only A wrote is exactly +0 again
                    assert not torch.signbit(g[k][only_a]).any(), (variant, k)
        e = check_pool_state(ops, g)
        ptrs.append(g["means"].data_ptr())
        print(f"{variant} step {i} ({cam}): {int(e.dirty.sum())} of {s.n} rows dirty")
        del g, e
    # steps 2 and 3 ran on the recycled buffer of step 1 (its gradients had been dropped)
    assert len(set(ptrs)) == 1 and len(entries(ops)) == 1


def test_gradients_the_caller_keeps_do_not_change(gs, oracle, dev, ops):
    s, ref = scene(gs, oracle, dev, "deg3")
    kept = s.step("A")
    g2 = s.step("B")                                                             # A's buffer is in use: a fresh one
    assert g2["means"].data_ptr() != kept["means"].data_ptr()
    same(g2, ref["B"], "B beside a kept A")
    same(kept, ref["A"], "kept A after B")
    view, kept_ptr, b_ptr = kept["sh"][10:20], kept["means"].data_ptr(), g2["means"].data_ptr()
    want = view.clone()
    del kept, g2
    g3 = s.step("A")                                    # one view still holds A's storage: B's buffer is the free one
    same(g3, ref["A"], "A again")
    assert torch.equal(view, want) and g3["means"].data_ptr() == b_ptr != kept_ptr
    check_pool_state(ops, g3)


def test_an_in_place_op_on_the_gradients_is_not_inherited(gs, oracle, dev, ops):
    s, ref = scene(gs, oracle, dev, "deg3")
    g = s.step("A")
    g["means"].mul_(2.0)
    g["sh"].add_(1.0)                                                            # no row of this buffer is zero any more
    del g
    g2 = s.step("B")
    same(g2, ref["B"], "B after an in-place op on A's gradients")
    check_pool_state(ops, g2)
    del g2
    same(s.step("A"), ref["A"], "A on B's recycled buffer")


def test_n_changes_between_frames(gs, oracle, dev, ops):
    s, ref = scene(gs, oracle, dev, "deg3")
    small = 3001                                                                 # one full chunk and an odd partial one
    ref_small = s.reference("B", first=small)
    same(s.step("A"), ref["A"], "N = 5000")
    g = s.step("B", first=small)
    assert g["means"].shape[0] == small
    same(g, ref_small, "N = 3001")
    check_pool_state(ops, g)
    del g
    same(s.step("B", first=small), ref_small, "N = 3001, recycled")
    same(s.step("A"), ref["A"], "N = 5000 again")
    assert all(e.shape_key[0] == N for e in entries(ops))


def _grid_scene(oracle):
    """rows 0..2047 (chunk 0): a grid of small translucent splats two pixels apart, all in view — every row of the chunk
    gets a gradient; rows 2048..4095 (chunk 1): behind the camera, no row ever touched; rows 4096..4999 (the partial
    chunk): 40 in view, the rest behind"""
    sc = oracle.synthetic_scene(N, W, H, sh_degree=3, seed=11, scale_mult=1.0)
    z, fx = 4.0, sc["fx"]
    means = sc["means"].clone()
    means[:, 2] = -5.0                                                           # behind the camera
    ix = torch.arange(2048)
    px = 2.0 * (ix % 46).float() + 2.5
    py = 1.75 * (ix // 46).float() + 1.5                                         # 45 rows of 46: 1.5 .. 78.5 of 80
    grid = torch.stack([(px - sc["cx"]) * z / fx, (py - sc["cy"]) * z / sc["fy"], torch.full((2048,), z)], -1)
    means[:2048] = grid
    means[4096:4136] = grid[torch.arange(40) * 50] + torch.tensor([0.0, 0.0, -1.0])
    sc["means"] = means
    sc["log_scales"] = torch.full((N, 3), math.log(1.5 * z / fx))                # sigma = 1.5 px
    sc["opacity_logits"] = torch.full((N,), math.log(0.1 / 0.9))
    sc["lin_vel"], sc["ang_vel"] = sc["lin_vel"] * 0.01, sc["ang_vel"] * 0.01
    return sc


def test_streamed_clean_and_sparse_chunks_in_one_frame(gs, oracle, dev, ops):
    s = Scene(gs, oracle, dev, "deg3", sc=_grid_scene(oracle))
    ref = {c: s.reference(c) for c in ("A", "A2")}
    g = s.step("A")
    same(g, ref["A"], "grid, fresh")
    e = check_pool_state(ops, g)
    dirty = e.dirty.bool()
    assert bool(dirty[:2048].all())                      # every row of chunk 0: the recycled step streams zeros over it
    assert not bool(dirty[2048:4096].any())              # chunk 1 has no dirty row
    assert 0 < int(dirty[4096:].sum()) <= (N - 4096) // 4     # the partial chunk zeroes row by row
    del g, e
    for i, cam in enumerate(("A2", "A", "A2")):          # (A2: the camera turned by 0.6 degrees — other values, same rows)
        g = s.step(cam)
        same(g, ref[cam], ("grid, recycled", i, cam))
        assert not g["means"][2048:4096].any() and not g["sh"][2048:4096].any()
        check_pool_state(ops, g)
        del g
    assert len(entries(ops)) == 1


def test_render_step_and_the_autograd_route_agree_on_pooled_buffers(gs, oracle, dev, ops):
    s, ref = scene(gs, oracle, dev, "deg3")
    sc = s.sc
    same(s.step("B"), ref["B"], "B")                     # leaves a recyclable entry with B's rows dirty
    names = ("means", "log_scales", "quats", "opacity_logits", "sh", "lin_vel", "ang_vel")
    q = {k: s.p[k].clone().requires_grad_(True) for k in names}
    vm = s.cams["A"].clone().requires_grad_(True)
    vms = gs.subpose_viewmats(vm, q["lin_vel"], q["ang_vel"], s.times)
    rgb, _, _ = gs.render_combined(q["means"], q["log_scales"], q["quats"], q["opacity_logits"], q["sh"], vms, None, S, 1,
                                   sc["fx"], sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0,
                                   return_alpha=False, raw_params=True)
    rgb.backward(s.wt)
    for k, name in (("means", "means"), ("log_scales", "scales"), ("quats", "quats"), ("opacity_logits", "opacities"),
                    ("sh", "sh")):
        assert torch.equal(q[k].grad, ref["A"][name]), k
    # (camera-level gradients: the bar tests/test_gpu_parity.py::test_render_step_equals_autograd_route holds them to)
    for got, name in ((vm.grad, "viewmat"), (q["lin_vel"].grad, "lin_vel"), (q["ang_vel"].grad, "ang_vel")):
        want = ref["A"][name]
        assert float((got - want).abs().max() / want.abs().max()) < 1e-5, name
    assert all(int(e.touched.count_nonzero()) == 0 for e in entries(ops))
    # the parameters' .grad hold the pooled storage: the next step must leave them alone
    same(s.step("B"), ref["B"], "B beside the .grad of A")
    assert torch.equal(q["sh"].grad, ref["A"]["sh"])
