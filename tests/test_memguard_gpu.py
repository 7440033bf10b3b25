"""GPU memory contract: every launch of the binding on poisoned, guarded memory.

tests/memguard.py's arena stands in for torch.empty / torch.empty_like while an op runs, so the
workspace, every plan buffer and every output come filled with zeros, with 0xFF (NaN floats,
-1 indices) or with what a run of the same op at identical shapes on another problem left
there, each between two 4096-B guard bands (test_memguard_cpu.py proves the helper).  Per op and
regime: the result meets the bound or restatement its own test uses (numerics.within with the
case's bound, no new tolerance; integers exactly), the guards are intact, the inputs unchanged;
and the three results are bitwise equal wherever the header calls the sum order fixed (every
forward form, csc, csc with edge_sel, dense, top-k, every plan, every integer output) -- pull,
bsort, hybrid and atomic sum through order-dependent atomics and get the bound only.

The other problem ("primer") of a stale run: the graph mirrored (column c -> C - 1 - c: the same
row_ptr and num_e) with other weights, values and selectors, where the allocation sizes depend
on the shapes alone; the same structure with other weights, values and selectors where they
follow the graph's contents (mode "auto" resolves through its locality, the hybrid's workspace
is sized by its plan's tile and edge counts).  memguard raises if the sizes differ after all.

An undersized workspace (size query - 1) is rejected on the host with "workspace too small"
before anything is launched: nothing in the arena is written.  (Found by this test:
maxk_bsort_plan ran its bucket plan, which needs less workspace, and wrote bucket_ptr,
bucket_pos and bucket_dst before its own check rejected the call.)
"""
import functools

import numpy as np
import pytest
import torch

import memguard as M
import numerics as N
import oracle as O
from conftest import GOLDEN, load_golden
from test_numerics_gpu import (BWD, BWD_IDS, CHUNKS, FWD, FWD_IDS, case, check_form, graph,
                               quiet_bsort, run_bwd, run_fwd)
from test_parity_gpu import T, bsort_layout, close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# graph Dn (E = 64e3) through a two-phase backward holds E * k * 4 bytes of contribution rows
# beside its plan and outputs: 4.1 MB at the table's k = 16 (the largest use, 5.5 MB with the
# guards), 8.4 MB should a k = 32 row join it; four times that.  Exhaustion raises.
ARENA_BYTES = 32 << 20


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@pytest.fixture(scope="module")
def arena(cuda):
    a = M.Arena(ARENA_BYTES, cuda)
    yield a
    print(f"\nmemguard: largest arena use {a.peak} B of {a.buf.numel()}")


# ------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def mirrored(name):
    """(col, ev) of the graph with column c sent to C - 1 - c and other weights: the same row_ptr
    and num_e, columns still ascending within a row."""
    g = graph(name)
    col = np.concatenate([(g.C - 1 - g.col[a:b])[::-1] for a, b in zip(g.rp[:-1], g.rp[1:])]
                         + [np.zeros(0, np.int32)]).astype(np.int32)
    ev = np.random.default_rng(31).uniform(0.5, 1.5, col.size).astype(np.float32)
    return col, ev


def graph_tensors(name, primer=False, mirror=True):
    """Fresh device tensors (rp, col, ev, div) of the graph, or of the primer's."""
    g = graph(name)
    col, ev = g.col, g.ev
    if primer:
        col, ev = mirrored(name)
        if not mirror:
            col = g.col
    return tuple(T(a, DEV) for a in (g.rp, col, ev, g.div))


@functools.lru_cache(maxsize=None)
def primer_case(name, D, k):
    g = graph(name)
    rng = np.random.default_rng(977 + D * 100 + k)
    return dict(ci=N.selectors(rng, g.C, D, k), cv=N.values(rng, (g.C, k), "unit"),
                G=N.values(rng, (g.R, D), "unit"), pre=N.values(rng, (g.R, D), "unit"))


def fill_independent(res, what):
    """The three regimes' outputs are the same bytes."""
    z = list(M.tensors(res["zero"]))
    for regime in ("stale", "ones"):
        o = list(M.tensors(res[regime]))
        assert len(o) == len(z)
        for i, (a, b) in enumerate(zip(z, o)):
            assert M.same_bytes(a, b), f"{what}: output {i} differs between zero and {regime}"


def npy(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("fid,family,name,D,k,variant", FWD, ids=FWD_IDS)
def test_forward(mk, arena, fid, family, name, D, k, variant):
    """Every forward form, whole and with the hub rows in slabs (slab_row, the fixups), written
    and accumulated onto a prefill in an arena `out`; emit's edge_sel_out from the arena;
    records with cbsr_records under the arena too."""
    check_form(mk, fid, name, D, k)
    c, p, g = case(name, D, k, "unit"), primer_case(name, D, k), graph(name)

    def factory(primer):
        s = p if primer else c
        return (graph_tensors(name, primer), T(s["cv"], DEV), T(s["ci"], DEV), T(s["pre"], DEV))

    for chunk in CHUNKS:
        for acc in (False, True):
            def op(gt, cv, ci, pre):
                out = es = None
                if acc:
                    out = torch.empty(g.R, D, dtype=torch.float32, device=DEV)
                    out.copy_(pre)
                if variant == "emit":
                    es = torch.empty(gt[1].numel(), k, dtype=torch.uint8, device=DEV)
                y = run_fwd(mk, name, variant, cv, ci, D, chunk, out=out, accumulate=acc, gt=gt,
                            es_out=es)
                assert arena.owns(y) and (out is None or y is out)
                return (y,) if es is None else (y, es)
            res = M.run_regimes(op, factory, arena)
            what = f"{fid} chunk {chunk}" + (" accumulate" if acc else "")
            for regime, r in res.items():
                N.within(r[0], c["ya" if acc else "yo"], c["bya" if acc else "by"],
                         f"{what} {regime}")
                if variant == "emit":
                    assert np.array_equal(npy(r[1]), c["ci"][g.col]), f"{what} {regime}"
            fill_independent(res, what)


# ------------------------------------------------------------------------------- backward
@quiet_bsort
@pytest.mark.parametrize("bid,family,name,D,k,mode,chunk,extra", BWD, ids=BWD_IDS)
def test_backward(mk, arena, bid, family, name, D, k, mode, chunk, extra):
    """Every backward mode, its plan (transpose, dense, bsort, pull, hybrid; cached on the fresh
    graph tensors or built with cache=False), edge_selectors and scaled entries built under the
    arena with it."""
    c, p = case(name, D, k, "unit"), primer_case(name, D, k)
    mirror = mode not in ("auto", "hybrid")

    def factory(primer):
        s = p if primer else c
        return (graph_tensors(name, primer, mirror), T(s["G"], DEV), T(s["ci"], DEV))

    def op(gt, G, ci):
        gs = run_bwd(mk, name, G, ci, mode, chunk, extra, gt=gt)
        assert arena.owns(gs)
        return gs
    res = M.run_regimes(op, factory, arena)
    for regime, gs in res.items():
        N.within(gs, c["go"], c["bg"], f"{bid} {regime}")
    if mode in ("csc", "dense"):
        fill_independent(res, bid)


# ------------------------------------------------------------------------------- plans
def plan_factory(name, mirror=True):
    return lambda primer: (graph_tensors(name, primer, mirror),)


def rows_of(g):
    return np.repeat(np.arange(g.R), np.diff(g.rp))


@pytest.mark.parametrize("name", ["S", "R"])
def test_transpose_and_dense_plan(mk, arena, name):
    g = graph(name)

    def op(gt):
        rp, col, ev, _ = gt
        return (mk.transpose_plan(col, g.C, cache=False),
                mk.dense_plan(rp, col, ev, g.C, cache=False))
    res = M.run_regimes(op, plan_factory(name), arena)
    order = np.argsort(g.col, kind="stable")  # CSC slot t holds CSR edge order[t]
    col_ptr = np.searchsorted(g.col[order], np.arange(g.C + 1))
    for regime, ((cp, eid), (cp2, t_src, t_w)) in res.items():
        assert np.array_equal(npy(cp), col_ptr) and np.array_equal(npy(cp2), col_ptr), regime
        assert np.array_equal(npy(eid), order), regime
        assert np.array_equal(npy(t_src), rows_of(g)[order]), regime
        assert np.array_equal(npy(t_w), g.ev[order]), regime
    fill_independent(res, "transpose / dense plan")


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("name", ["S", "R"])
def test_bsort_plan(mk, arena, name, k):
    g = graph(name)
    col = g.col.astype(np.int64)
    res = M.run_regimes(lambda gt: mk.bsort_plan(gt[0], gt[1], g.C, k, cache=False),
                        plan_factory(name), arena)
    for regime, (bptr, bpos, bdst, wsrc, wrow, shift) in res.items():
        assert shift == mk._lib().maxk_bucket_shift(k)
        W = mk._lib().maxk_bsort_window(k)
        nb = (g.C + (1 << shift) - 1) >> shift
        perm, pos = bsort_layout(col, k, shift, W, nb)
        order = np.argsort(col >> shift, kind="stable")
        assert np.array_equal(npy(bptr), np.searchsorted(col[order] >> shift, np.arange(nb + 1)))
        assert np.array_equal(npy(bdst).astype(np.int64), col[order] & ((1 << shift) - 1)), regime
        assert np.array_equal(npy(bpos), pos[order]), regime
        assert np.array_equal(npy(wsrc).astype(np.int64), perm - np.arange(col.size) // W * W)
        assert np.array_equal(npy(wrow), rows_of(g)), regime
    fill_independent(res, "bsort plan")


def check_pull_plan(mk, g, k, S, plan):
    tptr, ent, shift, s_ = plan
    assert s_ == S and shift == mk._lib().maxk_pull_shift(k)
    col = g.col.astype(np.int64)
    nb = (g.C + (1 << shift) - 1) >> shift
    rps = -(-g.R // S)
    key = (rows_of(g) // rps) * nb + (col >> shift)
    order = np.argsort(key, kind="stable")
    assert np.array_equal(npy(tptr), np.searchsorted(key[order], np.arange(S * nb + 1)))
    e = npy(ent).view(np.uint32)
    assert np.array_equal(e[:, 0] & 0xffff, rows_of(g)[order] % rps)
    assert np.array_equal(e[:, 0] >> 16, col[order] & ((1 << shift) - 1))
    assert np.array_equal(e[:, 1].view(np.float32), g.ev[order])
    return order, key[order], nb, rps


@pytest.mark.parametrize("k,S", [(4, 1), (16, 3), (16, 50)])
@pytest.mark.parametrize("name", ["S", "R"])
def test_pull_plan_and_scaled_entries(mk, arena, name, k, S):
    """pull_plan, and _scaled_entries over it: each weight divided by its source row's row_div,
    the key words unchanged."""
    g = graph(name)

    def op(gt):
        rp, col, ev, div = gt
        plan = mk.pull_plan(rp, col, ev, g.C, k, slices=S, cache=False)
        sc = mk._scaled_entries(plan[1], None, plan[0], g.R, g.C, plan[2], S, div)
        assert arena.owns(sc) and arena.owns(plan[1])
        return plan, sc
    res = M.run_regimes(op, plan_factory(name), arena)
    for regime, (plan, sc) in res.items():
        order, tile, nb, rps = check_pull_plan(mk, g, k, S, plan)
        s = npy(sc).view(np.uint32)
        assert np.array_equal(s[:, 0], npy(plan[1]).view(np.uint32)[:, 0]), regime
        rows = tile // nb * rps + (s[:, 0] & 0xffff)
        assert np.array_equal(rows, rows_of(g)[order])
        assert np.array_equal(s[:, 1].view(np.float32), g.ev[order] / g.div[rows]), regime
    fill_independent(res, "pull plan")


@pytest.mark.parametrize("density", [0.0, 0.5, 3.0, 1e9])  # all, most, the hub tiles, none
def test_hybrid_plan(mk, arena, density):
    """maxk_hybrid_plan against the numpy restatement of test_hybrid_plan_against_numpy, its pull
    plan and the csc part's transpose plan built under the arena with it."""
    name, k, D = "S", 16, 256
    g = graph(name)

    def op(gt):
        rp, col, ev, _ = gt
        return (mk.pull_plan(rp, col, ev, g.C, k, D, cache=False),
                mk.hybrid_plan(rp, col, ev, g.C, k, D, density=density, cache=False))
    # a mirrored graph has other tile counts, so another csc part: sizes differ at 0 < d < 1e9
    res = M.run_regimes(op, plan_factory(name, mirror=density in (0.0, 1e9)), arena)
    for regime, (pull, hyb) in res.items():
        tptr, ent, shift, S = pull
        tl, te, bp, bt, ent_d, shift2, S2, (oip, oix, oval, (ocp, oeid)) = hyb
        assert (shift2, S2) == (shift, S)
        check_pull_plan(mk, g, k, S, pull)
        nb = -(-g.C // (1 << shift))
        rps = -(-g.R // S)
        cnt = np.diff(npy(tptr).astype(np.int64))
        t_all = np.arange(S * nb)
        rows_in = np.clip(g.R - (t_all // nb) * rps, 1, rps)
        dense = (cnt > 0) & (cnt >= density * rows_in)
        want_tl = np.nonzero(dense)[0]
        assert np.array_equal(npy(tl), want_tl), regime
        assert np.array_equal(npy(te), np.concatenate([[0], np.cumsum(cnt[want_tl])])), regime
        j = want_tl % nb
        assert np.array_equal(npy(bp), np.concatenate([[0], np.cumsum(np.bincount(j, minlength=nb))]))
        assert np.array_equal(npy(bt), np.argsort(j * S + want_tl // nb, kind="stable")), regime
        tp, e = npy(tptr), npy(ent)
        want = np.concatenate([e[tp[t]:tp[t + 1]] for t in want_tl]) if want_tl.size else e[:0]
        assert np.array_equal(npy(ent_d), want), regime
        keep = ~dense[(rows_of(g) // rps) * nb + (g.col.astype(np.int64) >> shift)]
        assert np.array_equal(npy(oip), np.concatenate(
            [[0], np.cumsum(np.bincount(rows_of(g)[keep], minlength=g.R))])), regime
        assert np.array_equal(npy(oix), g.col[keep]) and np.array_equal(npy(oval), g.ev[keep])
        order = np.argsort(g.col[keep], kind="stable")
        assert np.array_equal(npy(ocp), np.searchsorted(g.col[keep][order], np.arange(g.C + 1)))
        assert np.array_equal(npy(oeid), order), regime
        if density == 0.0:
            assert oix.numel() == 0
        if density == 1e9:
            assert tl.numel() == 0 and oix.numel() == g.col.size
    fill_independent(res, "hybrid plan")


@pytest.mark.parametrize("name", ["S", "R"])
def test_pull_locality(mk, arena, name):
    g = graph(name)
    shift = int(mk._lib().maxk_pull_shift(16))
    res = M.run_regimes(lambda gt: torch.tensor(mk.pull_locality(gt[0], gt[1], shift),
                                                dtype=torch.float64),
                        plan_factory(name), arena)
    b = g.col.astype(np.int64) >> shift
    new = np.ones(b.size, bool)
    new[1:] = b[1:] != b[:-1]
    new[g.rp[:-1][np.diff(g.rp) > 0]] = True
    for regime, loc in res.items():
        assert abs(float(loc) - b.size / new.sum()) < 1e-9, regime
    fill_independent(res, "pull locality")
    assert len(arena.allocs) == 1 and arena.allocs[0].nbytes == 8  # its 8-B counter


@pytest.mark.parametrize("name", ["S", "R"])
def test_warp4(mk, arena, name):
    g = graph(name)

    def op(gt):
        w4 = mk.build_warp4_metadata(gt[0], 64)
        return w4, mk.warp4_to_indptr(w4, g.R)
    res = M.run_regimes(op, lambda primer: ((T(primer_rp(name) if primer else g.rp, DEV),),),
                        arena)
    for regime, (w4, back) in res.items():
        assert np.array_equal(npy(w4), O.warp4(g.rp, 64)), regime
        assert np.array_equal(npy(back), g.rp), regime
    fill_independent(res, "warp4")


@functools.lru_cache(maxsize=None)
def primer_rp(name):
    """Another row_ptr of the same length with the same number of warp4 entries (the schedule's
    size): the degrees of the rows in reverse order."""
    g = graph(name)
    rp = np.zeros_like(g.rp)
    rp[1:] = np.cumsum(np.diff(g.rp)[::-1])
    assert O.warp4(rp, 64).size == O.warp4(g.rp, 64).size
    return rp


@pytest.mark.parametrize("k", [3, 4, 16])
def test_edge_selectors(mk, arena, k):
    g = graph("S")
    ci = {pr: N.selectors(np.random.default_rng(k + 50 * pr), g.C, 256, k) for pr in (0, 1)}
    res = M.run_regimes(lambda gt, c: mk.edge_selectors(gt[1], c),
                        lambda primer: (graph_tensors("S", primer), T(ci[int(primer)], DEV)),
                        arena)
    for regime, es in res.items():
        assert np.array_equal(npy(es), ci[0][g.col]), regime
    fill_independent(res, "edge selectors")


# ------------------------------------------------------------------------------- top-k family
TOPK = [(257, 256, 16), (5, 7, 7), (131, 100, 10), (64, 64, 32)]  # the four-row kernel's tails,
TOPK_IDS = [f"V{v}-D{d}-k{k}" for v, d, k in TOPK]                # the non-vector path


@functools.lru_cache(maxsize=None)
def topk_data(V, D, k, primer):
    rng = np.random.default_rng(V * 7 + D + k + 1000 * primer)
    x = rng.standard_normal((V, D)).astype(np.float32)
    x[0] = np.round(x[0] * 2) / 2  # ties
    cv, ci = O.topk(x, k)
    return dict(x=x, cv=cv, ci=ci, xu=rng.integers(0, 256, (V, D)).astype(np.uint8),
                gv=rng.standard_normal((V, k)).astype(np.float32),
                gd=rng.standard_normal((V, D)).astype(np.float32))


def bits_equal(t, ref):
    return np.array_equal(npy(t).view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("V,D,k", TOPK, ids=TOPK_IDS)
def test_topk_encode(mk, arena, V, D, k):
    """topk_cbsr on fp32 (with the int32 selectors) and on uint8 input, topk_cbsr_dense on a
    contiguous and on a strided input, and the scatter to dense."""
    d = topk_data(V, D, k, 0)

    def factory(primer):
        s = topk_data(V, D, k, int(primer))
        wide = np.zeros((V, D + 5), np.float32)
        wide[:, :D] = s["x"]
        return T(s["x"], DEV), T(s["xu"], DEV), T(wide, DEV), T(s["cv"], DEV), T(s["ci"], DEV)

    def op(x, xu, wide, cv, ci):
        return (mk.topk_cbsr(x, k, with_int32=True), mk.topk_cbsr(xu, k),
                mk.topk_cbsr_dense(x, k), mk.topk_cbsr_dense(wide[:, :D], k),
                mk.cbsr_scatter_dense(cv, ci, D))
    res = M.run_regimes(op, factory, arena)
    order = np.lexsort((np.tile(np.arange(D), (V, 1)), -d["xu"].astype(np.int32)), axis=1)[:, :k]
    dense = O.scatter_dense(d["cv"], d["ci"], D)
    for regime, ((v, i, i32), (vu, iu), fused, fused_strided, sd) in res.items():
        assert bits_equal(v, d["cv"]) and np.array_equal(npy(i), d["ci"]), regime
        assert np.array_equal(npy(i32), d["ci"].astype(np.int32)), regime
        assert np.array_equal(npy(iu), order.astype(np.uint8)), regime
        assert np.array_equal(npy(vu), np.take_along_axis(d["xu"], order, 1)), regime
        for dn, v2, i2 in (fused, fused_strided):
            assert bits_equal(dn, dense) and bits_equal(v2, d["cv"]), regime
            assert np.array_equal(npy(i2), d["ci"]), regime
        assert bits_equal(sd, dense), regime
    fill_independent(res, "top-k encode")


@pytest.mark.parametrize("V,D,k", TOPK, ids=TOPK_IDS)
def test_topk_backward(mk, arena, V, D, k):
    """grad_x = scatter(grad_val + grad_dense[sel]): each of grad_val and grad_dense absent, both,
    and out= aliasing grad_dense (a copy of the input made in the arena)."""
    d = topk_data(V, D, k, 0)

    def factory(primer):
        s = topk_data(V, D, k, int(primer))
        return T(s["gv"], DEV), T(s["gd"], DEV), T(s["ci"], DEV)

    def op(gv, gd, ci):
        alias = torch.empty_like(gd)
        alias.copy_(gd)
        assert arena.owns(alias)
        return (mk.topk_backward(gv, None, ci, D), mk.topk_backward(None, gd, ci, D),
                mk.topk_backward(gv, gd, ci, D), mk.topk_backward(gv, alias, ci, D, out=alias))
    res = M.run_regimes(op, factory, arena)
    picked = np.take_along_axis(d["gd"], d["ci"].astype(np.int64), 1)
    want = [O.scatter_dense(w, d["ci"], D) for w in (d["gv"], picked, d["gv"] + picked)]
    for regime, outs in res.items():
        for got, w in zip(outs, want + want[2:]):
            assert bits_equal(got, w), regime
    fill_independent(res, "top-k backward")


@pytest.mark.parametrize("k", [16, 32])
def test_topk_u8_reference_unfilled_slots(mk, arena, k):
    """cuda_topk_maxk(reference_compat=True) at D = 256: slots never filled are 0, which only a
    poisoned output can tell from memory that happened to hold zeros."""
    def data(primer):
        rng = np.random.default_rng(k + 9 * primer)
        x = rng.integers(0, 256, (257, 256)).astype(np.uint8)
        x[:100] = rng.integers(0, 4, (100, 256)).astype(np.uint8) * 60  # 4 values, heavy ties
        x[100] = 77                                                      # nothing above the threshold
        x[101, 31::32] = 255                                             # the lane-31 overwrite
        return x
    res = M.run_regimes(lambda x: mk.cuda_topk_maxk(x, k, reference_compat=True),
                        lambda primer: (T(data(int(primer)), DEV),), arena)
    vo, io = O.topk_u8_reference(data(0), k)
    assert (vo == 0).any()  # rows with unfilled slots exist
    for regime, (v, i) in res.items():
        assert np.array_equal(npy(v), vo) and np.array_equal(npy(i), io), regime
    fill_independent(res, "uint8 reference top-k")


# ------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("fixture", ["tiny_d64_k4", "sym_d256_k16"])
@pytest.mark.parametrize("via", ["v1", "v4"])
def test_autograd(cuda, arena, via, fixture):
    """Forward and backward through maxk_spgemm (v1) and the MaxKSpmmWrapper v4 path under the
    arena, against the fixture as test_autograd_v1_golden / _v4_wrapper_golden compare."""
    import maxk_spgemm_function as F
    z = load_golden(f"{GOLDEN}/{fixture}.npz")
    k, D = int(z["k"]), int(z["D"])

    def factory(primer):
        rng = np.random.default_rng(5)
        x, g, tv = z["x"], z["g"], z["topk_val"]
        if primer:  # the same graph, other activations and gradients
            x, g, tv = (rng.permutation(a, axis=0) for a in (x, g, tv))
        return tuple(T(a, DEV) for a in (z["col_idx"], z["val"], z["row_ptr"], z["deg"], x, tv,
                                         z["topk_idx"], g))

    def op(col, val, ip, deg, x, tv, ti, g):
        if via == "v1":
            leaf = x.clone().requires_grad_(True)
            y = F.maxk_spgemm(col, val, leaf, k, graph_indptr=ip, in_degrees=deg, out_degrees=deg)
        else:
            w = F.MaxKSpmmWrapper("memguard")
            assert w.build_metadata(ip)
            leaf = tv.clone().requires_grad_(True)
            y = w.spmm(col, val, leaf, ti.long(), ip, deg, dim_origin=D)
        assert arena.owns(y)
        y.backward(g)
        return y, leaf.grad
    res = M.run_regimes(op, factory, arena)
    ref = (O.scatter_dense(z["grad_cbsr_ref"], z["topk_idx"], D) if via == "v1"
           else z["grad_cbsr_ref"])
    for regime, (y, grad) in res.items():
        close(y, z["y_ref"])
        close(grad, ref)


# ------------------------------------------------------------------------------- undersized
class Shrunk:
    """mk._L with one size query answering one byte less (or, for maxk_pull_locality, whose 8
    bytes have no query, the launch told of one byte less); every other attribute forwarded."""

    def __init__(self, lib, name):
        self._lib, self._name, self.sizes = lib, name, []

    def __getattr__(self, attr):
        f = getattr(self._lib, attr)
        if attr != self._name:
            return f
        if attr == "maxk_pull_locality":
            def launch(*a):
                self.sizes.append(a[7])
                return f(*a[:7], a[7] - 1, *a[8:])
            return launch

        def size(*a):
            n = int(f(*a))
            self.sizes.append(n)
            return n - 1
        return size


def _sspmm(mode, D=256, k=16, **kw):
    def prepare(mk, gt, c):
        rp, col, ev, _ = gt
        C = c["ci"].shape[0]
        plan = {"csc": lambda: mk.transpose_plan(col, C, cache=False),
                "bsort": lambda: mk.bsort_plan(rp, col, C, k, cache=False),
                "pull": lambda: mk.pull_plan(rp, col, ev, C, k, D, cache=False),
                "dense": lambda: mk.dense_plan(rp, col, ev, C, cache=False),
                "hybrid": lambda: mk.hybrid_plan(rp, col, ev, C, k, D, cache=False, **kw),
                "atomic": lambda: None}[mode]()
        G, ci = T(c["G"], DEV), T(c["ci"], DEV)
        # no row_div: the pull and the hybrid would first write their scaled entries
        return lambda: mk.sspmm_backward(rp, col, ev, G, ci, mode=mode, plan=plan)
    return D, k, prepare


def _forward(records):
    def prepare(mk, gt, c):
        rp, col, ev, div = gt
        cv, ci = T(c["cv"], DEV), T(c["ci"], DEV)
        D, k = c["G"].shape[1], c["ci"].shape[1]
        if records:
            rec = mk.cbsr_records(cv, ci, D)
            return lambda: mk.spgemm_forward_records(rp, col, ev, rec, k, D, row_div=div)
        return lambda: mk.spgemm_forward(rp, col, ev, cv, ci, D, row_div=div)
    return prepare


def _plan(build):
    return lambda mk, gt, c: (lambda: build(mk, gt, c["ci"].shape[0]))


# id: (the size query shrunk, D, k, prepare(mk, graph tensors, case) -> the launch, the arena
# allocations of the launch's own earlier steps)
UNDERSIZED = {
    "forward": ("maxk_spgemm_forward_workspace_size", 256, 16, _forward(False), 0),
    "forward-records": ("maxk_spgemm_forward_workspace_size", 256, 32, _forward(True), 0),
    "forward-dense": ("maxk_spgemm_forward_workspace_size", 64, 32, _forward(False), 0),
    "bwd-atomic": ("maxk_sspmm_backward_workspace_size", *_sspmm("atomic"), 0),
    "bwd-csc": ("maxk_sspmm_backward_csc_workspace_size", *_sspmm("csc"), 0),
    "bwd-bsort": ("maxk_sspmm_backward_bsort_workspace_size", *_sspmm("bsort"), 0),
    "bwd-pull": ("maxk_sspmm_backward_pull_workspace_size", *_sspmm("pull"), 0),
    "bwd-hybrid": ("maxk_sspmm_backward_hybrid_workspace_size", *_sspmm("hybrid", density=0.5), 0),
    "bwd-hybrid-inline": ("maxk_sspmm_backward_hybrid_workspace_size",
                          *_sspmm("hybrid", density=0.0), 0),
    "bwd-dense": ("maxk_sspmm_backward_dense_workspace_size", *_sspmm("dense", 64, 32), 0),
    "transpose-plan": ("maxk_transpose_plan_workspace_size", 256, 16,
                       _plan(lambda mk, gt, C: mk.transpose_plan(gt[1], C, cache=False)), 0),
    "bsort-plan": ("maxk_bsort_plan_workspace_size", 256, 16,
                   _plan(lambda mk, gt, C: mk.bsort_plan(gt[0], gt[1], C, 16, cache=False)), 0),
    "pull-plan": ("maxk_pull_plan_workspace_size", 256, 16,
                  _plan(lambda mk, gt, C: mk.pull_plan(gt[0], gt[1], gt[2], C, 16, cache=False)),
                  0),
    # its pull plan is built first, in the same call: tile_ptr, entries and their workspace
    "hybrid-plan": ("maxk_hybrid_plan_workspace_size", 256, 16,
                    _plan(lambda mk, gt, C: mk.hybrid_plan(gt[0], gt[1], gt[2], C, 16,
                                                           cache=False)), 3),
    "pull-locality": ("maxk_pull_locality", 256, 16,
                      _plan(lambda mk, gt, C: mk.pull_locality(gt[0], gt[1], 7)), 0),
    "warp4-build": ("maxk_warp4_build_workspace_size", 256, 16,
                    _plan(lambda mk, gt, C: mk.build_warp4_metadata(gt[0], 64)), 0),
}


@quiet_bsort
@pytest.mark.parametrize("uid", list(UNDERSIZED))
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, uid):
    """A workspace one byte short of the size query: RuntimeError "workspace too small" from
    the host-side check, before any launch -- the arena's outputs (0xFF-filled) are byte for
    byte unchanged and the guards intact.

    The atomic backward's documented size is 0 bytes (NULL is enough), so no workspace is one
    byte short of it: its case pins that 0 and that the launch is right on poisoned memory."""
    query, D, k, prepare, earlier = UNDERSIZED[uid]
    g, c = graph("S"), case("S", D, k, "unit")
    launch = prepare(mk, graph_tensors("S"), c)  # plans: real sizes
    torch.cuda.synchronize()
    if uid == "bwd-atomic":
        assert getattr(mk._lib(), query)(g.R, g.C, g.col.size, D, k, 0) == 0
        gs = M.run_once(arena, "ones", lambda: launch(), ())
        free = g._replace(div=None)  # the launch of these cases takes no row_div
        N.within(gs, N.bwd_ref(free, c["G"], c["ci"]), N.bound_bwd(free, c["G"], c["ci"]), uid)
        return
    shrunk = Shrunk(mk._L, query)
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            launch()
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made > earlier  # the launch's outputs and its short workspace came from the arena
    arena.check()
    assert arena.untouched(first=earlier)
