"""The gradient pool's decisions (ops._grad_pool_acquire / _grad_pool_commit / grad_pool_invalidate), on CPU tensors and
with a stub in place of the projection backward: when may the buffer of an earlier step be handed out again with only
its dirty rows zeroed, and when must the step get a fresh one.  (What the kernel does with either is
tests/test_gpu_grad_pool.py.)"""
import pytest
import torch


N, P, K = 64, 2, 4
WIDTH = 3 + 3 + 4 + 1 + 3 * K


@pytest.fixture()
def ops(gs):
    from gsdeblur_amd import ops
    ops.release_arenas()
    yield ops
    ops.release_arenas()


def stub_launch(entry, rows, fail=False):
    """what gs_project_fused_bwd_pooled does to an entry, in torch-free terms (raw writes: no version bump): zero the
    dirty rows (a fresh entry: all of them), write `rows`, leave their map in dirty; touched goes back to zero"""
    if fail:
        raise RuntimeError("launch failed")
    flat = entry.flat.numpy().reshape(N, WIDTH)            # (numpy writes do not touch torch's version counter)
    dirty = entry.dirty.numpy()
    flat[dirty != 0] = 0.0
    dirty[:] = 0
    for r in rows:
        flat[r] = float(r + 1)
        dirty[r] = 1
    entry.touched.numpy()[:] = 0


def step(ops, rows, fail=False, n=N, p=P, k=K, split=False):
    """one pooled backward: acquire -> launch -> commit -> the caller's gradient tensor (a view of the entry's buffer)"""
    entry = ops._grad_pool_acquire("cpu", n, p, k, split)
    fresh = bool(entry.dirty.all())
    stub_launch(entry, rows, fail)
    ops._grad_pool_commit(entry)
    return entry, entry.flat.view(n, -1), fresh


def expect(grad, rows):
    want = torch.zeros(N, WIDTH)
    for r in rows:
        want[r] = float(r + 1)
    assert torch.equal(grad, want)


def test_a_dropped_gradient_is_recycled_with_only_its_dirty_rows_zeroed(ops):
    e1, g1, fresh1 = step(ops, [1, 5])
    assert fresh1
    expect(g1, [1, 5])
    ptr = e1.flat.data_ptr()
    del g1
    e2, g2, fresh2 = step(ops, [7])
    assert e2 is e1 and not fresh2 and e2.flat.data_ptr() == ptr
    expect(g2, [7])                                                     # rows 1 and 5 are exactly zero again
    assert int(e2.touched.sum()) == 0


def test_a_view_the_caller_kept_blocks_recycling_and_stays_as_it_was(ops):
    e1, g1, _ = step(ops, [2])
    kept = g1[2:4]                                                      # any view keeps the storage in use
    del g1
    e2, g2, fresh2 = step(ops, [9])
    assert e2 is not e1 and fresh2
    assert torch.equal(kept[0], torch.full((WIDTH,), 3.0)) and not kept[1].any()
    expect(g2, [9])
    # the first buffer is free again once the view goes: the next step may take either, never one that is still held
    del kept
    e3, g3, fresh3 = step(ops, [0])
    assert e3 is e1 and not fresh3
    expect(g3, [0])
    expect(g2, [9])


def test_a_grad_assigned_to_a_parameter_blocks_recycling(ops):
    prm = torch.nn.Parameter(torch.zeros(N, WIDTH))
    e1, g1, _ = step(ops, [3])
    prm.grad = g1
    del g1
    e2, _, fresh2 = step(ops, [4])
    assert e2 is not e1 and fresh2
    expect(prm.grad, [3])


def test_an_in_place_op_of_the_callers_retires_the_entry(ops):
    e1, g1, _ = step(ops, [1])
    g1.mul_(2.0)                                                        # e.g. gradient clipping: bumps the version
    del g1
    e2, g2, fresh2 = step(ops, [6])
    assert e2 is not e1 and fresh2
    expect(g2, [6])
    assert all(e is not e1 for es in ops._grad_pool.values() for e in es)


def test_a_changed_shape_key_gets_its_own_entry_and_drops_the_old_one(ops):
    e1, g1, _ = step(ops, [1])
    del g1
    for kw in (dict(n=N + 8), dict(p=P + 1), dict(k=K + 5), dict(split=True)):
        e2 = ops._grad_pool_acquire("cpu", kw.get("n", N), kw.get("p", P), kw.get("k", K), kw.get("split", False))
        assert e2 is not e1 and bool(e2.dirty.all())
        assert e2.flat.numel() == (11 + 3 * kw.get("k", K)) * kw.get("n", N)
        assert e2.touched.numel() == kw.get("p", P) * kw.get("n", N) and int(e2.touched.sum()) == 0
    # (the scene changed shape: the old entry's memory went back to the allocator)
    assert all(e is not e1 for es in ops._grad_pool.values() for e in es)


def test_a_failed_launch_never_returns_its_entry(ops):
    e1, g1, _ = step(ops, [1])
    del g1
    with pytest.raises(RuntimeError):
        step(ops, [2], fail=True)                                       # took e1 out of the pool, never committed it
    assert not e1.valid
    assert all(e is not e1 for es in ops._grad_pool.values() for e in es)
    e3, g3, fresh3 = step(ops, [8])
    assert e3 is not e1 and fresh3
    expect(g3, [8])


def test_the_exchange_invalidates_the_entry_that_owns_a_gradient(ops):
    e1, g1, _ = step(ops, [1])
    other = torch.zeros(4)
    ops.grad_pool_invalidate(other)                                     # not the pool's: nothing happens
    assert e1.valid
    ops.grad_pool_invalidate(g1[3:5])                                   # a raw-pointer writer goes for this storage
    assert not e1.valid
    del g1
    e2, g2, fresh2 = step(ops, [2])
    assert e2 is not e1 and fresh2
    expect(g2, [2])


def test_the_row_exchange_of_dp_reports_its_raw_writes(ops, monkeypatch):
    from gsdeblur_amd import dp
    seen = []
    monkeypatch.setattr(ops, "grad_pool_invalidate", lambda t: seen.append(t.data_ptr()))
    g = [torch.zeros(N, 3), torch.zeros(N, 4)]
    row_ops = dp._RowOps(g)
    row_ops.grads = g
    dp._RowOps._raw_write(row_ops)
    assert seen == [t.data_ptr() for t in g]
    import inspect
    for name in ("scatter_add", "scatter_add_payload"):
        src = inspect.getsource(getattr(dp._RowOps, name))
        assert src.index("_raw_write()") < src.index("gs_dp_scatter_add"), name


def test_release_arenas_drops_the_gradient_pools(ops):
    e1, g1, _ = step(ops, [1])
    del g1
    assert any(ops._grad_pool.values())
    ops.release_arenas()
    assert not any(ops._grad_pool.values())
    e2, _, fresh2 = step(ops, [1])
    assert e2 is not e1 and fresh2


def test_the_pool_keeps_at_most_two_entries_per_stream(ops):
    held = [step(ops, [i]) for i in range(4)]                           # four steps' gradients alive at once
    assert len({id(h[0]) for h in held}) == 4
    assert sum(len(es) for es in ops._grad_pool.values()) == 2
    for i, (_, g, _) in enumerate(held):
        expect(g, [i])
