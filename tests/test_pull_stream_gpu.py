"""GPU: the stream pull backward (maxk_pull_stream_plan, maxk_sspmm_backward_pull_stream) with
forced bucket counts on small graphs, against the fp64 oracle with the per-element bound of
tests/numerics.py, and its plan against a numpy restatement.

Graphs (built once, never modified):
  hub   900 x 900, average degree 20, row 3 a hub of 850 edges, row 4 empty, column 411 read by
        no edge.  18.8k entries: one bucket holds more than one barrier run of the kernel
        (16384 entries) and no multiple of a workgroup step (1024 entries); at 7 buckets every
        bucket holds 2.7k.
  rect  700 rows over 1500 columns, average degree 12 (num_rows != num_cols; two buckets at
        least at k >= 32, where a bucket holds 1024 columns).
  tail  700 x 1500, every edge into columns >= 1100: at k = 64 and 3 buckets the first bucket
        is clamped to the full 1024 columns and receives no edge.
  hubcol 700 x 1500, column 500 read by every row and two more edges per row: at 7 buckets one
        bucket is that column alone (width 1), with boundaries on both sides of it; every
        bucket holds fewer entries than one workgroup step.
"""
import functools

import numpy as np
import pytest
import torch

import memguard as M
import numerics as N
from conftest import golden_cases, load_golden
from test_parity_gpu import T

pytestmark = pytest.mark.gpu

FORCED = ((1, 1), (3, 5), (7, 1), (7, 5))  # (buckets, slices)
STEP = 1024    # entries per workgroup step: 16 waves x 64
RUN = 16384    # entries between two workgroup barriers (sspmm_pull.hip)


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


def _csr(rows, R):
    rp = np.zeros(R + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return rp, np.concatenate(rows).astype(np.int64)


@functools.lru_cache(maxsize=None)
def graph(name):
    rng = np.random.default_rng({"hub": 11, "rect": 12, "tail": 13, "hubcol": 14}[name])
    if name == "hub":
        V = 900
        deg = rng.poisson(20, V)
        deg[3], deg[4] = 850, 0
        rp, col = _csr([np.sort(rng.choice(V, d, replace=False)) for d in deg], V)
        return N.make_graph(rng, rp, col, V, unread=411)
    R, C = 700, 1500
    if name == "rect":
        rows = [np.sort(rng.choice(C, d, replace=False)) for d in rng.poisson(12, R)]
    elif name == "tail":
        rows = [1100 + np.sort(rng.choice(C - 1100, 6, replace=False)) for _ in range(R)]
    else:
        others = np.delete(np.arange(C), 500)
        rows = [np.sort(np.append(rng.choice(others, 2, replace=False), 500)) for _ in range(R)]
    rp, col = _csr(rows, R)
    return N.make_graph(rng, rp, col, C)


@functools.lru_cache(maxsize=None)
def problem(name, k, D, twist=True):
    """Selectors, G and the oracle's result and bound with and without row_div.  twist: one
    destination repeats a selector, and at D < 256 one selects column 200 >= D (reads 0)."""
    g = graph(name)
    rng = np.random.default_rng(1000 * k + D)
    ci = N.selectors(rng, g.C, D, k)
    if twist:
        dst = int(g.col[g.rp[g.hub]])  # a destination the hub row reaches
        ci[dst, 1] = ci[dst, 0]
        if D < 256:
            ci[int(g.col[g.rp[g.hub] + 1]), 2] = 200
    G = N.values(rng, (g.R, D), "unit")
    nd = g._replace(div=None)
    n = N.count_bwd(g, ci, D)
    return dict(g=g, ci=ci, G=G, n=n,
                ref={True: N.bwd_ref(g, G, ci), False: N.bwd_ref(nd, G, ci)},
                bound={True: N.bound_bwd(g, G, ci, n=n), False: N.bound_bwd(nd, G, ci, n=n)})


def dev_graph(g, cuda):
    return T(g.rp, cuda), T(g.col, cuda), T(g.ev, cuda)


def npy(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------- the plan
def check_plan(mk, g, k, nb, S, plan):
    """bucket_col, grp_ptr and the entries against numpy; returns (bucket_col, counts)."""
    shift = int(mk._lib().maxk_pull_shift(k))
    cap = 1 << shift
    assert (plan.shift, plan.n_buckets, plan.slices) == (shift, nb, S)
    bc = npy(plan.bucket_col).astype(np.int64)
    assert bc.shape == (nb + 1,) and bc[0] == 0 and bc[-1] == g.C
    w = np.diff(bc)
    assert (w >= 0).all() and (w <= cap).all(), w
    col = g.col.astype(np.int64)
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    bucket = np.searchsorted(bc, col, side="right") - 1
    rps = -(-g.R // S)
    key = bucket * S + rows // rps
    order = np.argsort(key, kind="stable")  # (bucket, slice, CSR order)
    e = npy(plan.ent).view(np.uint32)
    assert np.array_equal(e[:, 0] >> shift, rows[order])
    assert np.array_equal(e[:, 0] & (cap - 1), (col - bc[bucket])[order])
    assert np.array_equal(e[:, 1].view(np.float32), g.ev[order])
    assert np.array_equal(npy(plan.grp_ptr), np.searchsorted(bucket[order], np.arange(nb + 1)))
    return bc, np.diff(npy(plan.grp_ptr).astype(np.int64))


@pytest.mark.parametrize("nb,S", FORCED)
@pytest.mark.parametrize("name,k", [("hub", 8), ("hub", 16), ("hub", 64), ("rect", 16),
                                    ("rect", 32), ("hubcol", 64), ("tail", 64)])
def test_plan_against_numpy(mk, cuda, name, k, nb, S):
    g = graph(name)
    cap = 1 << int(mk._lib().maxk_pull_shift(k))
    if nb * cap < g.C:
        with pytest.raises(RuntimeError, match="do not cover"):
            mk.pull_stream_plan(*dev_graph(g, cuda), g.C, k, groups=nb, slices=S, cache=False)
        return
    plan = mk.pull_stream_plan(*dev_graph(g, cuda), g.C, k, groups=nb, slices=S, cache=False)
    bc, counts = check_plan(mk, g, k, nb, S, plan)
    indeg = np.bincount(g.col, minlength=g.C)
    print(f"{name} k={k} nb={nb}: widths {np.diff(bc).tolist()} counts {counts.tolist()} "
          f"max in-degree {indeg.max()}")
    if (np.diff(bc) < cap).all():
        # Every boundary is the column whose prefix count is nearest its share i * E / nb, so
        # it is off by at most half the in-degree of the column it falls in or next to: a
        # bucket's count differs from the equal share E / nb by at most the largest in-degree.
        assert np.abs(counts - g.col.size / nb).max() <= indeg.max(), (counts, indeg.max())


def test_corner_buckets(mk, cuda):
    """The graphs do produce the corners their docstring names."""
    L = mk._lib()
    cap64 = 1 << int(L.maxk_pull_shift(64))
    g = graph("tail")
    plan = mk.pull_stream_plan(*dev_graph(g, cuda), g.C, 64, groups=3, slices=1, cache=False)
    bc, counts = check_plan(mk, g, 64, 3, 1, plan)
    assert bc[1] - bc[0] == cap64 and counts[0] == 0  # full width, no edge
    g = graph("hubcol")
    plan = mk.pull_stream_plan(*dev_graph(g, cuda), g.C, 64, groups=7, slices=1, cache=False)
    bc, counts = check_plan(mk, g, 64, 7, 1, plan)
    b = int(np.searchsorted(bc, 500, side="right") - 1)
    assert bc[b] == 500 and bc[b + 1] == 501 and counts[b] == g.R  # the hub column alone
    assert 0 < counts.max() < STEP
    g = graph("hub")
    plan = mk.pull_stream_plan(*dev_graph(g, cuda), g.C, 16, groups=1, slices=1, cache=False)
    _, counts = check_plan(mk, g, 16, 1, 1, plan)
    assert counts[0] > RUN and counts[0] % STEP != 0 and counts[0] % RUN != 0


# ------------------------------------------------------------------------------- the backward
def run_stream(mk, cuda, p, k, nb, S, use_div):
    g = p["g"]
    rp, col, ev = dev_graph(g, cuda)
    plan = mk.pull_stream_plan(rp, col, ev, g.C, k, p["G"].shape[1], groups=nb, slices=S)
    return mk.sspmm_backward(rp, col, ev, T(p["G"], cuda), T(p["ci"], cuda),
                             row_div=T(g.div, cuda) if use_div else None, mode="pull", plan=plan,
                             validate=False)  # a selector >= D is one of the cases


@pytest.mark.parametrize("D", [256, 100])
@pytest.mark.parametrize("k", [8, 16, 32, 64])
def test_backward_against_oracle(mk, cuda, monkeypatch, k, D):
    """Every part layout (k = 8 one part of 8 values per lane, 16 two parts, 32 / 64 parts of
    16 slots), full and narrow D, 1 / 3 / 7 buckets, and the three row_div routes: none,
    weights pre-divided in the plan's entries, G / row_div written per call (gprime_kernel)."""
    p = problem("hub", k, D)
    for nb, S in FORCED:
        for route in ("none", "prescaled", "gprime"):
            monkeypatch.setenv("MAXK_PULL_PRESCALE", "0" if route == "gprime" else "1")
            div = route != "none"
            out = run_stream(mk, cuda, p, k, nb, S, div)
            q = N.within(out, p["ref"][div], p["bound"][div], f"k={k} D={D} nb={nb} S={S} {route}")
            print(f"k={k} D={D} nb={nb} S={S} {route}: err/bound {q:.3f}")


@pytest.mark.parametrize("name,k,nb", [("rect", 16, 1), ("rect", 16, 3), ("rect", 32, 3),
                                       ("rect", 64, 7), ("tail", 64, 3), ("hubcol", 64, 7),
                                       ("hubcol", 16, 7)])
def test_backward_rectangular_and_corners(mk, cuda, name, k, nb):
    """700 rows over 1500 columns; the bucket without edges (exact zeros: its bound is 0), the
    bucket of one column, full-width buckets, buckets below one workgroup step."""
    p = problem(name, k, 256, twist=False)
    for div in (True, False):
        out = run_stream(mk, cuda, p, k, nb, 5, div)
        N.within(out, p["ref"][div], p["bound"][div], f"{name} k={k} nb={nb} div={div}")
    if name == "tail":
        assert not npy(out)[:1100].any()


def test_backward_inf_nan(mk, cuda):
    p = problem("hub", 16, 100, twist=False)
    g = p["g"]
    rng = np.random.default_rng(77)
    cv = N.values(rng, p["ci"].shape, "unit")
    _, cip, Gp, _ = N.poison(g, cv, p["ci"], p["G"], 100)
    ref = N.bwd_ref(g, Gp, cip)
    N.reference_is_meaningful(ref)
    rp, col, ev = dev_graph(g, cuda)
    plan = mk.pull_stream_plan(rp, col, ev, g.C, 16, 100, groups=3, slices=5)
    out = mk.sspmm_backward(rp, col, ev, T(Gp, cuda), T(cip, cuda), row_div=T(g.div, cuda),
                            mode="pull", plan=plan, validate=False)
    N.within(out, ref, N.bound_bwd(g, Gp, cip), "poisoned")


def test_backward_golden_and_repeats(mk, cuda):
    """A golden graph through the stream path; two runs agree to fp32 rounding (fp64 sums, one
    rounding), as test_pull_backward_repeats asks of the tiled pull."""
    z = load_golden(next(c for c in golden_cases() if "sym_d256_k16" in c))
    rng = np.random.default_rng(5)
    g = N.make_graph(rng, z["row_ptr"].astype(np.int64), z["col_idx"].astype(np.int64))
    g = g._replace(ev=z["val"].astype(np.float32), div=z["deg"].astype(np.float32))
    assert g.C <= 1500
    G, ci = z["g"].astype(np.float32), z["topk_idx"]
    rp, col, ev = dev_graph(g, cuda)
    plan = mk.pull_stream_plan(rp, col, ev, g.C, 16, groups=3, slices=5)
    args = (rp, col, ev, T(G, cuda), T(ci, cuda))
    a = mk.sspmm_backward(*args, row_div=T(g.div, cuda), mode="pull", plan=plan)
    b = mk.sspmm_backward(*args, row_div=T(g.div, cuda), mode="pull", plan=plan)
    N.within(a, N.bwd_ref(g, G, ci), N.bound_bwd(g, G, ci), "golden")
    assert torch.allclose(a, b, rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------- routing
def test_rule_routes_mode_pull(mk, cuda, monkeypatch):
    """A Reddit-shaped table (232,965 columns, two edges per row) at k = 16: where the rule
    accepts the shape on this device, backward_plan and sspmm_backward take the stream path;
    MAXK_PULL_STREAM=0 keeps the tiled plan.  Both against the oracle."""
    V, D, k = 232965, 256, 16
    rng = np.random.default_rng(3)
    col = np.sort(rng.integers(0, V, (V, 2)), axis=1).reshape(-1)
    g = N.make_graph(rng, np.arange(V + 1, dtype=np.int64) * 2, col, V)
    ci = N.selectors(rng, V, D, k)
    G = N.values(rng, (V, D), "unit")
    rp, colt, ev = dev_graph(g, cuda)
    nb = mk.pull_stream_buckets(cuda, V, V, col.size, D, k)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert nb == int(mk._lib().maxk_pull_stream_buckets(V, V, col.size, D, k, cus))
    if cus == 256:
        assert nb == 128
    ref, bound = N.bwd_ref(g, G, ci), N.bound_bwd(g, G, ci)
    plan = mk.backward_plan(colt, V, k, "pull", indptr=rp, values=ev, dim=D)
    assert isinstance(plan, mk.PullStreamPlan) == (nb > 0)
    if nb:
        assert plan.n_buckets == nb
    out = mk.sspmm_backward(rp, colt, ev, T(G, cuda), T(ci, cuda), row_div=T(g.div, cuda),
                            mode="pull")
    N.within(out, ref, bound, "stream by rule")
    monkeypatch.setenv("MAXK_PULL_STREAM", "0")
    assert mk.pull_stream_buckets(cuda, V, V, col.size, D, k) == 0
    tiled = mk.backward_plan(colt, V, k, "pull", indptr=rp, values=ev, dim=D)
    assert not isinstance(tiled, mk.PullStreamPlan) and len(tiled) == 4
    out = mk.sspmm_backward(rp, colt, ev, T(G, cuda), T(ci, cuda), row_div=T(g.div, cuda),
                            mode="pull")
    N.within(out, ref, bound, "tiled by switch")


# ------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("name,k,nb", [("hub", 16, 3), ("rect", 64, 7)])
def test_guarded_poisoned_memory(mk, cuda, name, k, nb):
    """Plan, scaled entries and backward on workspaces and outputs of exactly the documented
    sizes between guard bands, zero-, stale- and 0xFF-filled (tests/memguard.py)."""
    p, p2 = problem(name, k, 256, twist=False), problem(name, k, 256, twist=True)
    g = p["g"]
    arena = M.Arena(64 << 20, cuda)

    def factory(primer):
        q = p2 if primer else p
        ev = g.ev[::-1].copy() if primer else g.ev
        return (T(g.rp, cuda), T(g.col, cuda), T(ev, cuda), T(q["G"], cuda), T(q["ci"], cuda),
                T(g.div, cuda))

    def op(rp, col, ev, G, ci, div):
        plan = mk.pull_stream_plan(rp, col, ev, g.C, k, groups=nb, slices=5, cache=False)
        assert arena.owns(plan.ent) and arena.owns(plan.bucket_col)
        a = mk.sspmm_backward(rp, col, ev, G, ci, row_div=div, mode="pull", plan=plan)
        b = mk.sspmm_backward(rp, col, ev, G, ci, mode="pull", plan=plan)
        return list(plan), a, b  # a list: memguard.copy_out rebuilds plain containers only
    res = M.run_regimes(op, factory, arena)
    for regime, (plan, a, b) in res.items():
        check_plan(mk, g, k, nb, 5, mk.PullStreamPlan(*plan))
        N.within(a, p["ref"][True], p["bound"][True], f"{regime} row_div")
        N.within(b, p["ref"][False], p["bound"][False], f"{regime} plain")
    ws = int(mk._lib().maxk_sspmm_backward_pull_stream_workspace_size(g.R, g.C, 256, k))
    assert ws in [a.nbytes for a in arena.allocs]
