"""GPU: the grid-stride kernels of the three newest families past their first round.

linear_maxk_kernel, x16_topk_kernel, x16_scatter_kernel and x16_pack_kernel loop over their work
under a grid cap and carry state between rounds (tests/test_rounds_cpu.py names it and guards
the sizes).  Every input here is built on the device from a small pool of distinct rows,
x = pool[kind], and compared with expected = ref[kind]: the CPU reference costs P rows, not V,
nothing large crosses the bus, and every comparison is of bytes.
"""
import numpy as np
import pytest
import torch

import memguard as M
import numerics as N
import test_linear_maxk_gpu as LM
import test_rounds_cpu as RC
import topk_rows as TR
import x16_ref as XR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T = LM.T


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


def kinds(V, P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, P, (V,), generator=g, device=DEV)


def first_of_kind(kind, P):
    """Per kind the first row holding it (every kind occurs: V >> P)."""
    rows = torch.arange(kind.numel(), device=DEV)
    first = torch.full((P,), kind.numel(), device=DEV).scatter_reduce_(0, kind, rows, "amin")
    assert int(first.max()) < kind.numel()
    return first


def same_rows(got, ref, kind, step=1 << 14):
    """got == ref[kind] in bytes, a block of rows at a time (no second [V, k] tensor)."""
    return all(M.same_bytes(got[s:s + step], ref[kind[s:s + step]])
               for s in range(0, kind.numel(), step))


# ------------------------------------------------------------------------------- fused layer
@pytest.mark.parametrize("I,D,k", RC.LM_SHAPES, ids=[LM.ids(s) for s in RC.LM_SHAPES])
def test_fused_layer_later_tiles(mk, I, D, k):
    """2 slots + 3 tiles over a grid of `slots` workgroups: every workgroup prefetches a second
    and a third tile's first slab under the epilogue of the one before, whose selection has
    just scribbled on the LDS the slab returns to.  Integer-valued operands (test_linear_maxk_
    gpu.case): bit-exact in any order."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    slots, n_tiles, V = RC.lm_sizes(cus)
    assert n_tiles > 2 * 2 * cus
    P = 257
    c = LM.case(P, I, D, k, "int", True)
    kind = kinds(V, P, 6000 + I + D + k)
    mk.topk_error_rows()
    vals, idx = mk.linear_maxk_forward(T(c["x"])[kind], T(c["W"]), T(c["b"]), k=k)
    assert M.same_bytes(vals, T(c["vals"].astype(np.float32))[kind])
    assert M.same_bytes(idx, T(c["idx"])[kind])
    first = first_of_kind(kind, P)  # equal rows in different tiles and rounds: equal bytes
    assert M.same_bytes(vals, vals[first[kind]]) and M.same_bytes(idx, idx[first[kind]])
    rounds = (torch.arange(V, device=DEV) // RC.lm_tile_rows() // slots)
    assert int((rounds[first[kind]] != rounds).sum()) > V // 2
    assert mk.topk_error_rows() == 0


# ------------------------------------------------------------------------------- x16 encode
def encode_inputs(D, k, tail):
    pool = TR.rows(D, np.random.default_rng(6100 + D))
    val, idx = XR.topk(pool, k)
    V = RC.topk_rows_total(tail)
    kind = kinds(V, len(pool), 6200 + D + tail)
    return pool, val, idx, kind


@pytest.mark.parametrize("tail", [1, 2, 3])
@pytest.mark.parametrize("D,k", RC.TOPK_SHAPES)
def test_encode_later_rounds(mk, cuda, D, k, tail):
    """Two full rounds of the capped grid, then a third whose last workgroup has 1-3 live waves;
    the next row's loads are issued while this row is ranked.  The pool is the hard-row corpus."""
    pool, val, idx, kind = encode_inputs(D, k, tail)
    x = T(pool)[kind]
    ref_v, ref_i = T(val), T(idx.astype(np.int16))
    mk.topk_error_rows(cuda)
    v, i = mk.topk_cbsr_x16(x, k)
    assert same_rows(v, ref_v, kind) and same_rows(i, ref_i, kind)
    del v, i
    if D < 1024:  # the dense form at the two narrower shapes: the widest stays near 0.7 GB
        dense, v, i = mk.topk_cbsr_dense_x16(x, k)
        assert same_rows(v, ref_v, kind) and same_rows(i, ref_i, kind)
        assert M.same_bytes(dense, torch.zeros_like(x).scatter_(1, i.long(), v))
    assert mk.topk_error_rows(cuda) == 0


# ------------------------------------------------------------------------------- x16 adjoint
@pytest.mark.parametrize("D,k,tail", [(257, 33, 2), (384, 16, 3)])
def test_adjoint_later_rounds(mk, cuda, D, k, tail):
    """x16_scatter_kernel over the same rows (D = 257: scalar stores, 384: 16-byte stores), its
    LDS row reused every round: the three forms, and in place over grad_dense."""
    pool, _, _, kind = encode_inputs(D, k, tail)
    sel = mk.topk_cbsr_x16(T(pool)[kind], k)[1]
    V, it = sel.shape[0], sel.long()
    g = torch.Generator(device=DEV).manual_seed(6300 + D)
    gv = torch.randn(V, k, generator=g, device=DEV)
    gd = torch.randn(V, D, generator=g, device=DEV)
    for a, b in ((gv, None), (None, gd), (gv, gd)):
        src = (0 if a is None else a) + (0 if b is None else b.gather(1, it))
        want = torch.zeros(V, D, device=DEV).scatter_(1, it, src)
        assert M.same_bytes(mk.topk_backward_x16(a, b, sel, D), want)
    buf = gd.clone()
    out = mk.topk_backward_x16(gv, buf, sel, D, out=buf)
    assert out.data_ptr() == buf.data_ptr() and M.same_bytes(buf, want)


# ------------------------------------------------------------------------------- x16 pack
def pack_case(D, k):
    """64 rows of about 20 source vertices out of C = 2 rounds + 3 (row 0 a hub of 300), the
    vertices at both ends of every round read by some row; the CBSR from a pool of 97 records
    by vertex number, a repeated selector planted in one read vertex of each round.  The
    reference runs on the compacted set of the vertices the edges read."""
    rng = np.random.default_rng(6400 + D)
    C, rnd, P = RC.pack_cols_total(k), RC.pack_round_cols(k), 97
    ends = [0, rnd - 1, rnd, 2 * rnd - 1, 2 * rnd, C - 1]
    lists = [rng.integers(0, C, 300 if r == 0 else 20) for r in range(64)]
    lists[0][:6] = ends
    for r, v in enumerate(ends):
        lists[1 + r][0] = v
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    col = np.concatenate(lists)
    pool_v = rng.standard_normal((P, k), dtype=np.float32)
    pool_i = XR.topk(rng.standard_normal((P, D), dtype=np.float32), k)[1]
    dup = (0, rnd, C - 1)  # slot 1 repeats slot 0's selector: the pack folds it
    used, inv = np.unique(col, return_inverse=True)
    cv, ci = pool_v[used % P].copy(), pool_i[used % P].copy()
    ci[np.searchsorted(used, dup), 1] = ci[np.searchsorted(used, dup), 0]
    g = N.make_graph(rng, rp, inv.reshape(-1), len(used))
    return dict(g=g, C=C, col=col, pool_v=pool_v, pool_i=pool_i, dup=dup, P=P,
                fwd=XR.fwd(g, cv, ci, D), bound=XR.bound_fwd(g, cv, ci, D))


@pytest.mark.parametrize("D,k,vpb", RC.PACK_SHAPES, ids=[f"D{d}-k{k}" for d, k, _ in RC.PACK_SHAPES])
def test_pack_later_rounds(mk, cuda, D, k, vpb):
    """x16_pack_kernel past its grid cap: records of the second and third round (s_bits and
    s_dup zeroed again, a repeated selector in each round), read by x16_fwd_kernel at the auto
    item size and at 64 tokens (the hub row continues in a slab)."""
    c = pack_case(D, k)
    g, C = c["g"], c["C"]
    kind = torch.arange(C, device=DEV) % c["P"]
    cv, ci = T(c["pool_v"])[kind], T(c["pool_i"].astype(np.int16))[kind]
    dup = T(np.array(c["dup"]))
    ci[dup, 1] = ci[dup, 0]
    rp, col, ev, div = (T(a) for a in (g.rp, c["col"].astype(np.int32), g.ev, g.div))
    bound, n = c["bound"]
    assert (n == 0).any() and (n > 1).any()
    for chunk in (0, 64):
        out = mk.spgemm_forward_x16(rp, col, ev, cv, ci, D, row_div=div, chunk=chunk,
                                    validate=False)
        r = N.within(out, c["fwd"], bound, f"pack D{D} k{k} chunk {chunk}")
        print(f"pack D{D} k{k} C{C} chunk {chunk}: err/bound {r:.3f}")
        assert not out[T(n == 0)].view(torch.int32).any()
        again = mk.spgemm_forward_x16(rp, col, ev, cv, ci, D, row_div=div, chunk=chunk,
                                      validate=False)
        assert M.same_bytes(out, again)
