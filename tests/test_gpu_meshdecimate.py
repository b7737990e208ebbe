"""Mesh decimation on the GPU: the kernels of csrc/meshdecimate.hip against the numpy reference of
tests/meshdecimate_reference.py and, bit for bit, against the host build of csrc/meshdecimate_math.h.

Comparison (meshdecimate_reference.assert_same): every integer equal (cluster_of, faces', all counts, the vertex and face
order, the chosen ladder index); positions and colours within 2 float32 ulps of max(|value|, s) of the reference — derived
there, not measured; the kernels and the host build give the same bits.  No case is excluded.  Sizes are the smallest at
which each piece can go wrong: below, at and above one and four 256-thread blocks."""
import functools

import numpy as np
import pytest
import torch

import meshdecimate_reference as R
import test_gpu_streams as S
import test_meshdecimate_host as H
import tsdf_reference as T

pytestmark = pytest.mark.gpu
mh, delay, streams, recorder = H.mh, S.delay, S.streams, S.recorder          # fixtures of the host and the stream tests


def to_gpu(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(a).to(dev) for a in arrays)


def gpu_decimate(gs, dev, verts, faces, colors, s, **kw):
    out = gs.mesh_decimate(*to_gpu(dev, verts, faces, colors), cell_size=s, return_map=True, return_stats=True, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[3].dtype == torch.int32
    assert all(t.is_cuda for t in (out[0], out[1], out[3])) and tuple(out[0].shape[1:]) == (3,) == tuple(out[1].shape[1:])
    return out[0].cpu().numpy(), out[1].cpu().numpy(), None if out[2] is None else out[2].cpu().numpy(), out[3].cpu().numpy(), out[4]


def same_bits(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


def check(mh, gs, dev, verts, faces, colors, s, what, ref=None, **kw):
    """the kernels against the reference (tolerance) and the host build (bits) -> (the kernels' result, the reference's)"""
    ref = ref or R.decimate(verts, faces, colors, s, **kw)
    got = gpu_decimate(gs, dev, verts, faces, colors, s, **kw)
    used = ref[4]["cell_size"]
    R.assert_same(got, ref, used, what)
    assert got[4]["cell_size"] == used and got[4]["plans"] == ref[4]["plans"]
    host = H.host_decimate(mh, verts, faces, colors, used, kw.get("dedupe", True))
    assert all(same_bits(g, h) for g, h in zip(got[:4], host[:4])), what + ": the kernels and the host build differ in bits"
    return got, ref


@functools.lru_cache(maxsize=None)
def sphere_reference(key, s, target):
    verts, faces = SPHERE[key]
    return R.decimate(verts, faces, None, s, target_faces=target)


SPHERE = {}


@pytest.fixture(scope="module")
def sphere(gs, dev):
    """the 48^3 ray-cast sphere of the TSDF tests, fused and extracted by the kernels -> (verts, faces, voxel, centre, radius)"""
    origin, vs, dims, depth, views, intr, trunc, center, radius = T.e2e_scene(48)
    vol = gs.TSDFVolume(origin, vs, dims, device=dev, color=False)
    gs.tsdf_integrate(vol, *to_gpu(dev, depth, views, intr), trunc)
    verts, faces, _ = gs.tsdf_extract_mesh(vol)
    SPHERE["e2e"] = (verts.cpu().numpy(), faces.cpu().numpy())
    return SPHERE["e2e"] + (vs, center, radius)


# ---- 1: weld --------------------------------------------------------------------------------------------------------------------
def test_weld(mh, gs, dev):
    verts, faces = R.cube_soup()
    got, _ = check(mh, gs, dev, verts, faces, None, 0.125, "cube")
    assert got[0].shape == (8, 3) and got[1].shape == (12, 3) and got[4]["clusters"] == 8
    assert R.ulp_error(got[0][got[3]], verts, 0.125) <= 2.0            # three planes meet at every corner


# ---- 2: plane -------------------------------------------------------------------------------------------------------------------
def test_plane(mh, gs, dev):
    verts, faces = R.plane(32)
    got, ref = check(mh, gs, dev, verts, faces, None, 2.0, "plane")
    assert got[4]["clusters"] == 289 == len(got[0]) and not got[0][:, 2].any()
    means = np.stack([verts[got[3] == c].astype(np.float64).mean(0) for c in range(289)])
    assert R.ulp_error(got[0][:, :2], means[:, :2], 2.0) <= 2.0
    assert len(got[1]) == len(ref[1]) and np.array_equal(got[1], ref[1])


# ---- 3: everything collapses ----------------------------------------------------------------------------------------------------
def test_everything_collapses(mh, gs, dev):
    verts, faces = R.tetrahedron()
    got, _ = check(mh, gs, dev, verts, faces, None, 1.0, "tetrahedron")
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[4]["degenerate"] == 4 and (got[3] == -1).all()
    assert got[4]["verts_out"] == 0 and got[4]["faces_out"] == 0 and got[4]["clusters"] == 1


# ---- 4: block edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,F", R.EDGE_SIZES)
def test_block_edges(mh, gs, dev, V, F):
    verts, faces, colors = R.soup(V, F)
    for dedupe in (True, False):
        got, _ = check(mh, gs, dev, verts, faces, colors, 0.5, f"soup {V} {F} dedupe {dedupe}", dedupe=dedupe)
        assert got[4]["faces_out"] + got[4]["degenerate"] + got[4]["duplicates"] == F
    check(mh, gs, dev, verts, faces, None, 0.5, f"soup {V} {F} without colours")


# ---- 5: sphere ------------------------------------------------------------------------------------------------------------------
def test_sphere(mh, gs, dev, sphere):
    verts, faces, vs, center, radius = sphere

    def radial(v):
        return float(np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(center), axis=1) - radius).max())
    refs = [(k, sphere_reference("e2e", k * vs, None)) for k in (2.0, 1.5, 3.0)]
    for k, ref in refs:
        print(f"sphere at {k} voxels: F {len(faces)} -> {len(ref[1])}, V {len(verts)} -> {len(ref[0])}, edge uses "
              f"{R.edge_counts(ref[1])}, closed genus 0 {R.is_closed_genus0(ref[0], ref[1])}, reference radial error "
              f"{radial(verts):.5f} -> {radial(ref[0]):.5f} (voxel {vs:.5f})")
    closed = [(k, ref) for k, ref in refs if R.is_closed_genus0(ref[0], ref[1])]
    k, ref = closed[0] if closed else refs[0]
    got, _ = check(mh, gs, dev, verts, faces, None, k * vs, f"sphere {k}", ref=ref)
    if closed:
        assert R.is_closed_genus0(got[0], got[1])
    else:
        uses = R.edge_counts(got[1])
        assert uses == R.edge_counts(ref[1]) and sum(n for e, n in uses.items() if e != 2) > 0


# ---- 6: target_faces ------------------------------------------------------------------------------------------------------------
def test_target_faces(mh, gs, dev, sphere):
    verts, faces, vs = sphere[:3]
    for N in (len(faces) // 4, len(faces) // 20):
        ref = sphere_reference("e2e", vs, N)
        got, _ = check(mh, gs, dev, verts, faces, None, vs, f"target {N}", ref=ref, target_faces=N)
        print(f"target {N}: index {ref[4]['index']}, F' {got[4]['faces_out']}, plans {got[4]['plans']}")
        assert got[4]["faces_out"] <= N and 2 <= got[4]["plans"] <= 8 and ref[4]["index"] > 0
        assert got[4]["cell_size"] == vs * 2.0 ** (ref[4]["index"] / 4)
    ref = sphere_reference("e2e", vs, len(faces))                      # P(0) already holds
    got, _ = check(mh, gs, dev, verts, faces, None, vs, "target met at once", ref=ref, target_faces=len(faces))
    assert ref[4]["index"] == 0 and got[4]["plans"] == 1 and got[4]["cell_size"] == vs
    v, f = R.octant_faces()
    check(mh, gs, dev, v, f, None, 1.0, "octants", target_faces=1)
    with pytest.raises(ValueError, match="not reached"):
        gpu_decimate(gs, dev, v, f, None, 1.0, target_faces=0)
    with pytest.raises(ValueError, match="target_faces"):
        gpu_decimate(gs, dev, v, f, None, 1.0, target_faces=-1)


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_fault(mh, gs, dev):
    """the kernels test every index and every coordinate before they use it and leave a status word: a guarded read, no
    address is formed from the bad value"""
    V, F = 600, 700
    verts, faces, colors = R.soup(V, F)
    for bad in (-1, V):
        f = faces.copy()
        f[311, 1] = bad
        for kw in (dict(), dict(dedupe=False), dict(target_faces=100)):
            with pytest.raises(ValueError, match="outside"):
                gpu_decimate(gs, dev, verts, f, colors, 0.5, **kw)
    for bad in (float("nan"), 1e30, -float("inf")):
        v = verts.copy()
        v[123, 1] = bad
        with pytest.raises(ValueError, match="not finite or more than"):
            gpu_decimate(gs, dev, v, faces, colors, 0.5)
    check(mh, gs, dev, verts, faces, colors, 0.5, "the same process's next call")


# ---- 8: determinism -------------------------------------------------------------------------------------------------------------
def test_same_bits_every_run_whatever_memory_held(gs, dev, sphere, streams):
    soup = to_gpu(dev, *R.soup(1023, 1025))
    ball = to_gpu(dev, sphere[0], sphere[1])

    def run():
        a = gs.mesh_decimate(*soup, cell_size=0.5, return_map=True)
        b = gs.mesh_decimate(*ball, cell_size=sphere[2], target_faces=len(sphere[1]) // 20, return_map=True)
        return [t.cpu().numpy() for t in a + b if t is not None]
    first, second = run(), run()
    assert all(same_bits(x, y) for x, y in zip(first, second))
    S.poison_free_memory(dev, streams)            # the workspace and every output come out of 0xFF-filled blocks
    third = run()
    assert all(same_bits(x, y) for x, y in zip(first, third))


# ---- 9: side stream -------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream_while_the_default_stream_is_busy(gs, dev, sphere, streams, delay, recorder):
    """the method of tests/test_gpu_streams.py: warm up on the side stream, two idle-stream runs bit-equal as the
    reference, poison, then run behind a busy default stream; the run counts only if the delay's event has not completed at
    the last fetch.  The entry points take their stream from the descriptor, so they are not in that file's table."""
    import time
    soup = to_gpu(dev, *R.soup(1023, 1025))
    ball = to_gpu(dev, sphere[0], sphere[1])

    def run():
        names = ("verts", "faces", "colors", "cluster_of")
        a = gs.mesh_decimate(*soup, cell_size=0.5, return_map=True)
        b = gs.mesh_decimate(*ball, cell_size=sphere[2], target_faces=len(sphere[1]) // 20, return_map=True)
        out = {"soup_" + n: t for n, t in zip(names, a)}
        out.update({"ball_" + n: t for n, t in zip(names, b) if t is not None})
        return out
    s = streams[0]
    with torch.cuda.stream(s):
        S.fetch(run())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = S.fetch(run())
    wall_ms = (time.perf_counter() - t0) * 1e3
    again = S.fetch(run())
    torch.cuda.synchronize()
    assert not S.differing(ref, again), "not bit-reproducible on an idle stream"
    d_ms = max(4.0 * wall_ms, S.MIN_DELAY_MS)
    S.poison_free_memory(dev, streams)
    recorder.clear()
    try:
        got, still_busy = S.run_behind_busy_default(dev, delay, s, d_ms, run)
        print(f"mesh_decimate: wall {wall_ms:.2f} ms, delay {d_ms:.1f} ms, valid {still_busy}")
        assert still_busy, "the delay on the default stream had ended before the results were fetched: the run proves nothing"
        assert not S.differing(got, ref)
        assert {"gs_mesh_decimate_plan", "gs_mesh_decimate_emit"} <= recorder.names()
    finally:
        torch.cuda.synchronize()


# ---- 10: the export tool ----------------------------------------------------------------------------------------------------------
def test_export_tool_on_the_generated_dataset(gs, dev, tmp_path, monkeypatch, capsys):
    """tools/export_mesh.py over the self-generated dataset of tools/train_deblur.py --generate (as
    tests/test_gpu_tsdf.py::test_export_mesh_tool makes it): twice without the new flags (the same bytes), with
    --keep-largest 1 --target-faces N (the README's line) and with --decimate-cell.  The tool's main() runs in this
    process with its own argument parsing (one process start for the training, none per export).  A decimated file must
    hold gs.mesh_decimate of the plain file's (cleaned) mesh: positions and faces equal; a colour may differ by one 8-bit
    level, because the file holds colours rounded to 8 bits, the mean of values that are each at most half a level off is
    at most half a level off, and two numbers half a level apart round to levels at most one apart."""
    import importlib.util
    import json
    import subprocess
    import sys
    data = tmp_path / "scene"
    subprocess.check_call([sys.executable, str(H.ROOT / "tools" / "train_deblur.py"), "--generate", str(data), "--width", "96",
                           "--height", "64", "--frames", "8", "--gaussians", "2000", "--blur-samples", "0", "--iterations",
                           "30", "--export-ply", "--out", str(tmp_path / "run")], cwd=str(tmp_path))
    spec = importlib.util.spec_from_file_location("export_mesh_tool_gpu", H.ROOT / "tools" / "export_mesh.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    capsys.readouterr()

    def export(name, *flags):
        out = tmp_path / name
        monkeypatch.setattr(sys, "argv", ["export_mesh.py", "--ply", str(tmp_path / "run" / "splat_blur_samples_0.ply"), "--data",
                                          str(data), "--set", "all", "--resolution", "64", "--out", str(out), *flags])
        tool.main()
        return out, json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    def levels(c):
        return torch.round(c.clamp(0, 1) * 255).to(torch.int32)
    plain, line = export("plain.ply")
    again, line2 = export("again.ply")
    assert plain.read_bytes() == again.read_bytes()
    assert not {"decimate_cell", "clusters", "faces_before_decimation"} & set(line) and line["faces"] == line2["faces"] > 0
    vs = line["voxel_size"]
    verts, faces, colors = (t.to(dev) for t in gs.tsdf.read_mesh_ply(plain))
    assert len(faces) == line["faces"]
    # the README's line: clean, then decimate from the voxel size upwards
    cv, cf, cc = gs.mesh_filter_components(verts, faces, colors, keep_largest=1)
    N = len(cf) // 4
    small, sline = export("small.ply", "--keep-largest", "1", "--target-faces", str(N))
    wv, wf, wc, stats = gs.mesh_decimate(cv, cf, cc, cell_size=vs, target_faces=N, return_stats=True)
    gv, gf, gc = (t.to(dev) for t in gs.tsdf.read_mesh_ply(small))
    print(f"export_mesh: F {len(faces)}, cleaned {len(cf)}, --target-faces {N} -> {len(gf)} at cell {sline['decimate_cell']:.5f} "
          f"(voxel {vs:.5f})")
    assert torch.equal(gv, wv) and torch.equal(gf, wf) and 0 < len(gf) <= N
    assert int((levels(gc) - levels(wc)).abs().max()) <= 1
    assert sline["faces"] == len(gf) and sline["vertices"] == len(gv) and sline["kept"] == 1
    assert sline["decimate_cell"] == stats["cell_size"] > vs and sline["clusters"] == stats["clusters"]
    assert sline["faces_before_decimation"] == len(cf)
    # a fixed cell, no clean-up
    fixed, fline = export("fixed.ply", "--decimate-cell", repr(2 * vs))
    wv, wf, wc, stats = gs.mesh_decimate(verts, faces, colors, cell_size=2 * vs, return_stats=True)
    gv, gf, gc = (t.to(dev) for t in gs.tsdf.read_mesh_ply(fixed))
    assert torch.equal(gv, wv) and torch.equal(gf, wf) and 0 < len(gf) < len(faces)
    assert int((levels(gc) - levels(wc)).abs().max()) <= 1
    assert fline["decimate_cell"] == 2 * vs and fline["clusters"] == stats["clusters"] and "kept" not in fline
    assert fline["faces_before_decimation"] == len(faces)
