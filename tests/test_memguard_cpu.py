"""tests/memguard.py proved on a CPU arena with small fake ops written in torch: what the GPU
tests (test_memguard_gpu.py) rely on when they call a kernel's memory clean."""
import pytest
import torch

import memguard as M

N = 100  # floats per fake output: 400 B, so payload byte n is not on an alignment boundary


@pytest.fixture
def arena():
    return M.Arena(256 * 1024, "cpu")


def inputs(primer):
    g = torch.Generator().manual_seed(2 if primer else 1)
    return (torch.randn(N, generator=g),)


def clean(x):
    ws = torch.empty(3, 50, dtype=torch.float32)
    ws.copy_(x.view(2, 50)[:1].expand(3, 50))
    out = torch.empty(N)
    out.copy_(x * 2 + (ws[0] - ws[2]).repeat(2))
    return out


def test_clean_op_passes_every_regime(arena):
    res = M.run_regimes(clean, inputs, arena)
    assert list(res) == ["zero", "stale", "ones"]
    for regime, out in res.items():
        assert torch.equal(out, inputs(False)[0] * 2), regime
        assert not arena.owns(out)  # copied out
    assert arena.peak > 0 and arena.peak % M.ALIGN == 0


def test_views_have_the_asked_shape_dtype_and_alignment(arena):
    with arena.active("ones"):
        a = torch.empty(3, 5, dtype=torch.int32, device="cpu")
        b = torch.empty((7,), dtype=torch.uint8)
        c = torch.empty_like(a)
        d = torch.empty(0, 2, dtype=torch.float32)
        e = torch.empty(2, 2)
    assert a.shape == (3, 5) and a.dtype == torch.int32 and bool((a == -1).all())
    assert b.shape == (7,) and bool((b == 0xFF).all())
    assert c.shape == a.shape and c.dtype == a.dtype and c.data_ptr() != a.data_ptr()
    assert d.shape == (0, 2) and e.dtype == torch.get_default_dtype()
    for t in (a, b, c, e):
        assert arena.owns(t) and t.is_contiguous()
        assert (t.data_ptr() - arena.buf.data_ptr()) % M.ALIGN == 0
    assert [x.nbytes for x in arena.allocs] == [60, 7, 60, 0, 16]
    assert [x.ordinal for x in arena.allocs] == [0, 1, 2, 3, 4]
    assert all("test_memguard_cpu.py" in x.site and "test_views_have" in x.site
               for x in arena.allocs)
    arena.check()
    with arena.active("zero"):
        z = torch.empty(4, dtype=torch.float32)
    assert bool((z == 0).all())
    # the canary: a large negative float, a negative int32, no fill byte
    w = torch.full((4,), M.CANARY, dtype=torch.uint8)
    assert float(w.view(torch.float32)) < -1e38 and int(w.view(torch.int32)) < 0
    assert M.CANARY not in M.FILL.values()


def past_end(x):
    out = torch.empty(N)
    out.copy_(x)
    out.as_strided((N + 1,), (1,))[N] = 1.0  # payload byte n exactly
    return out


def before_start(x):
    first = torch.empty(8)
    first.zero_()
    out = torch.empty(N)
    out.copy_(x)
    out.as_strided((1,), (1,), out.storage_offset() - 1)[0] = 1.0  # one element before
    return out


def middle_slack(x):
    a, b, c = torch.empty(N), torch.empty(N, dtype=torch.int32), torch.empty(N)
    for t in (a, b, c):
        t.zero_()
    b.view(torch.uint8).as_strided((4 * N + 101,), (1,))[4 * N + 100] = 7  # b's slack
    return a


@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("op,ordinal,side,offset", [
    (past_end, 0, "after", 4 * N), (before_start, 1, "before", -4),
    (middle_slack, 1, "after", 4 * N + 100)], ids=["past-end", "before-start", "middle-slack"])
def test_guard_damage_is_located(arena, op, ordinal, side, offset, regime):
    if regime == "stale":
        M.run_once(arena, "zero", clean_like(op), inputs(True))
    with pytest.raises(M.GuardDamaged) as e:
        M.run_once(arena, regime, op, inputs(False))
    d = e.value
    assert (d.alloc.ordinal, d.side, d.offset) == (ordinal, side, offset)
    assert d.alloc.nbytes == 4 * N
    assert f"#{ordinal}" in str(d) and side in str(d) and str(offset) in str(d)
    assert "test_memguard_cpu.py" in d.alloc.site and op.__name__ in d.alloc.site


def clean_like(op):
    """The same allocation sizes as `op` without its stray store (the run a stale run follows)."""
    sizes = {past_end: [(N, torch.float32)], before_start: [(8, torch.float32), (N, torch.float32)],
             middle_slack: [(N, torch.float32), (N, torch.int32), (N, torch.float32)]}[op]

    def run(x):
        for n, dt in sizes:
            torch.empty(n, dtype=dt).zero_()
    return run


def stale_accumulator(x):
    """Adds a workspace into its result before anything in this run wrote it."""
    ws = torch.empty(N)
    out = torch.empty(N)
    out.copy_(x + ws)
    ws.copy_(x)  # scratch use afterwards: what the next run finds
    return out


def test_unwritten_float_shows_in_ones_and_stale(arena):
    res = M.run_regimes(stale_accumulator, inputs, arena)
    want = inputs(False)[0]
    assert torch.equal(res["zero"], want)
    assert torch.isnan(res["ones"]).all()
    assert torch.isfinite(res["stale"]).all() and not torch.equal(res["stale"], want)
    assert torch.equal(res["stale"], want + inputs(True)[0])


def slab_inputs(primer):
    """Six work items; each adds its slab into row `rows[i]`, the items with active[i] = 0 add
    nothing.  The primer's problem activates other items."""
    g = torch.Generator().manual_seed(4 if primer else 3)
    rows = torch.tensor([1, 2, 3, 1, 2, 3], dtype=torch.int32)
    active = torch.tensor([1, 1, 1, 0, 1, 0] if primer else [1, 0, 1, 1, 0, 1], dtype=torch.int32)
    return rows, active, torch.randn(6, 4, generator=g)


def slab_fixup(rows, active, slab):
    """The slab_row bug: an inactive item leaves its slot unwritten instead of storing -1, and
    the fixup reads every slot, treating a negative row as "nothing to do"."""
    slab_row = torch.empty(6, dtype=torch.int32)
    out = torch.empty(4, 4)
    out.zero_()
    for i in range(6):
        if active[i]:
            slab_row[i] = rows[i]
    for i in range(6):
        if slab_row[i] >= 0:
            out[int(slab_row[i])] += slab[i]
    return out


def test_unwritten_index_shows_in_zero_and_stale(arena):
    res = M.run_regimes(slab_fixup, slab_inputs, arena)
    rows, active, slab = slab_inputs(False)
    want = torch.zeros(4, 4)
    for i in range(6):
        if active[i]:
            want[int(rows[i])] += slab[i]
    assert torch.equal(res["ones"], want)       # -1: skipped, the bug hidden
    assert not torch.equal(res["zero"], want)   # 0: a valid row gets the slab
    assert not torch.equal(res["stale"], want)  # the primer's row for that item
    assert torch.isfinite(res["zero"]).all() and torch.isfinite(res["stale"]).all()


def test_modified_input_is_rejected(arena):
    def op(x):
        out = torch.empty(N)
        out.copy_(x)
        x[17] += 1.0
        return out
    with pytest.raises(M.InputModified, match="input #0"):
        M.run_once(arena, "zero", op, inputs(False))
    nan = (torch.full((N,), float("nan")),)  # NaN inputs compare equal to themselves
    M.run_once(arena, "zero", clean, nan)


def test_same_calls_same_offsets(arena):
    M.run_once(arena, "zero", clean, inputs(False))
    first = [(a.offset, a.nbytes) for a in arena.allocs]
    M.run_once(arena, "stale", clean, inputs(True))
    assert [(a.offset, a.nbytes) for a in arena.allocs] == first
    assert len(first) == 2 and all(o % M.ALIGN == 0 for o, _ in first)
    # bands of their own: a whole guard on either side of the 600-B and the 400-B payload
    assert first[0][0] == M.GUARD and first[1][0] == first[0][0] + M.ALIGN + 2 * M.GUARD


def test_stale_run_with_other_sizes_raises_before_it_runs(arena):
    M.run_once(arena, "zero", clean, inputs(False))

    def other(x):
        torch.empty(3, 50, dtype=torch.float32)
        torch.empty(N + 1)
    with pytest.raises(M.SequenceChanged, match="#1"):
        M.run_once(arena, "stale", other, inputs(False))
    with pytest.raises(M.SequenceChanged):
        M.Arena(8192, "cpu").begin("stale")  # nothing before it


def test_exhaustion_raises():
    small = M.Arena(4 * M.ALIGN, "cpu")
    with small.active("zero"):
        torch.empty(M.ALIGN, dtype=torch.uint8)  # guard + payload + guard: fits
        with pytest.raises(M.ArenaExhausted):
            torch.empty(1, dtype=torch.uint8)
    with small.active("zero"), pytest.raises(M.ArenaExhausted):
        torch.empty(2 * M.ALIGN + 1, dtype=torch.uint8)


def test_other_calls_pass_through_and_patch_is_undone(arena):
    orig, orig_like = torch.empty, torch.empty_like
    with arena.active("ones"):
        assert torch.empty is not orig and torch.empty_like is not orig_like
        pinned = torch.empty(16, dtype=torch.float32, pin_memory=False)
        meta = torch.empty(16, device="meta")
        strided = torch.empty(4, 4, memory_format=torch.contiguous_format)
        out = torch.empty(3, out=torch.zeros(3))
        like_meta = torch.empty_like(torch.zeros(4), device="meta")
        like_t = torch.empty_like(torch.zeros(4, 6).t())  # not contiguous: torch's own strides
        mine = torch.empty(16)
    assert meta.is_meta and like_meta.is_meta and like_t.stride() == (1, 6)
    for t in (pinned, strided, out, like_t):
        assert not arena.owns(t)
    assert arena.owns(mine) and len(arena.allocs) == 1
    assert torch.empty is orig and torch.empty_like is orig_like
    with pytest.raises(ZeroDivisionError):
        with arena.active("zero"):
            1 / 0
    assert torch.empty is orig and torch.empty_like is orig_like


def test_untouched_tells_a_run_that_wrote_nothing(arena):
    with arena.active("ones"):
        t = torch.empty(N)
    assert arena.untouched()
    t[3] = 0.5
    assert not arena.untouched()
