"""The corners of the row hand-out (csrc/token_items.h: RowHandout and its pointer window), on
the four kernels whose lane groups take an item's rows in order: the streaming forward
(stream_rows), the csc backward's grouped phase 2 (csc_groups), the dense route's walk
(dense_rows_body, which keeps the hand-out written out) and the dense backward's pick form
(pick_rows_kernel).

The variant suite gives every instantiation an empty row, ragged rows and a hub row; this file
aims one small graph at the hand-out itself.  handout_graph.handout_degrees() lists its rows, in
order:

  rows 0..139   0, 1 or 2 edges each, so at an item size of 512 tokens the first item hands out
                more than 128 rows and slides its 64-entry window twice (at rows 63 and 126);
                the rows at window positions 62, 63 and 64 of both slides hold edges;
  row 140, 141  exactly 64 and 65 edges: the last row the groups take and the first they
                refuse (MAXK_FWD_STREAM, kCscGroupMax and kDenseGroupMax are all 64);
  rows 142..145 a few dozen edges each, sized so that
  row 146       (5 edges) has the first item's last token, 511: under the cut-at-the-end rule
                its owner walks none of it, under the hub rule all of it, past the item's end;
  row 147       the hub, 1530 edges (about three items), ending on token 2047, so that
  row 148       has the token 2048 = the fourth item's end: it belongs to the fifth;
  rows 149..249 0 to 3 edges each; rows 250..259 empty, so the last item's hand-out runs into
                num_rows.

The graph is a symmetric multigraph (the rows' edge stubs paired at random, (a, b) giving a -> b
and b -> a; the hub mostly pairs with itself), so its transpose has the same pointer array and
the backward's walks over the CSC meet the same corners.  Every call runs at an explicit item
size of 512 and of 64 tokens (512 = 8 * 64, so both tokens above are item ends at either size);
at 64 the 65-edge row is a hub and the groups' length cap is the item size itself.

Comparison as in test_variants_gpu.py: the per-element bound of tests/numerics.py against the
fp64 oracle, N(0,1) and mixed-magnitude values, with row_div and without.  The selection check
(no GPU) shows, with the rules of tests/variant_cases.py, that each call launches the kernel
named.
"""
import functools

import numpy as np
import pytest

import numerics as N
import variant_cases as VC
from handout_graph import HUB_ROW, LAST_TOKEN_ROW, NEXT_ITEM_ROW, R, handout_csr, handout_degrees

D = 64
CHUNKS = (512, 64)

#  id            op       k    kernels the call launches
CASES = {
    "stream-k16": ("fwd", 16, ("spgemm_fwd_kernel<16, 8, false, false, true>",)),
    "stream-k32": ("fwd_records", 32, ("spgemm_fwd_kernel<32, 8, false, false, true>",)),
    "csc-k16": ("csc", 16, ("sspmm_bwd_kernel<4, 4, 2>",
                            "csc_sum_kernel<true, 64, 4, true, true, false>")),
    "csc-k32": ("csc", 32, ("sspmm_bwd_kernel<8, 4, 2>",
                            "csc_sum_kernel<true, 64, 4, true, true, true>")),
    "csc-k64": ("csc", 64, ("sspmm_bwd_kernel<16, 4, 2>",
                            "csc_sum_kernel<true, 64, 4, true, true, true>")),
    "dense-k32": ("dense", 32, ("dense_rows_kernel<16, 4>", "dense_select_rows_kernel<16, 4>")),
    "pick-k16": ("pick", 16, ("pick_rows_kernel<16, 4>",)),
}
PARAMS = [(cid, chunk) for cid in CASES for chunk in CHUNKS]


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def prepared(k):
    """The graph, selectors and addend counts at width k: built once, never modified."""
    rp, col = handout_csr()
    rng = np.random.default_rng(911 + k)
    g = N.make_graph(rng, rp, col, R)
    ci = N.selectors(rng, R, D, k)
    return dict(g=g, ci=ci, nf=N.count_fwd(g, ci, D), nb=N.count_bwd(g, ci, D))


# ------------------------------------------------------------------------------- no GPU
def test_graph_meets_the_corners():
    rp, col = handout_csr()
    deg = np.diff(rp)
    assert np.array_equal(deg, handout_degrees())
    assert np.array_equal(np.bincount(col, minlength=R), deg), "the transpose has the same rows"
    tok = np.arange(R) + rp[:-1]
    assert deg[:140].max() == 2 and {0, 1, 2} <= set(deg[:140].tolist())
    assert (deg[[62, 63, 64, 125, 126, 127]] > 0).all()
    assert tok[141] + 1 + 65 <= 512, "the first item of 512 tokens owns rows 0..141"
    assert (deg[140], deg[141]) == (64, 65)
    assert tok[LAST_TOKEN_ROW] == 511 and deg[LAST_TOKEN_ROW] > 0
    assert deg[HUB_ROW] > 2.9 * 512 and tok[HUB_ROW] + deg[HUB_ROW] == 2047
    assert tok[NEXT_ITEM_ROW] == 2048
    assert (deg[250:] == 0).all() and deg[149:250].max() == 3


def _case(cid, chunk):
    op, k, kernels = CASES[cid]
    vop = {"fwd": "wide_fwd", "fwd_records": "wide_fwd", "pick": "dense"}.get(op, op)
    hub = int(handout_degrees()[HUB_ROW])
    return VC.Case(cid, "handout", vop, k, D, R, R, 0, 0, hub, chunk, {}, kernels, "")


@pytest.mark.parametrize("cid,chunk", PARAMS)
def test_case_selects_its_kernels(cid, chunk):
    """variant_cases' restatement of the host rules names the kernels of the table above."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    K = VC.constants()
    op, k, kernels = CASES[cid]
    c = _case(cid, chunk)
    E = int(handout_csr()[0][-1])
    assert c.hub > chunk, "the hub row is split over items"
    if op == "pick":
        # dense_route.hip dense_pick: the backward mode "dense" below k = D / 2 picks columns
        assert 2 * k < D and k <= K["kWave"] and k % 4 == 0 and D % 4 == 0
        # ... and the library says so: the pick form's workspace holds slabs of k floats and no
        # dense Y of num_cols * D floats, which the row-selecting form's (k = 32 here) does
        size = L.maxk_sspmm_backward_dense_workspace_size
        assert size(R, R, E, D, k, chunk) < R * D * 4 <= size(R, R, E, D, 32, chunk)
        got = (f"pick_rows_kernel<{VC.lanes_per_edge(k, K['kWave'])}, {K['MAXK_DENSE_U']}>",)
    elif op == "fwd_records":
        # D = 64, k = 32 takes the dense route from cbsr tables; over transport records it is
        # the streaming forward
        assert L.maxk_records_ok(R, R, E, D, k) == 1
        got = (VC.fwd_kernel(c, E, K),)
    elif op == "fwd":
        assert L.maxk_dense_route(D, k) == 0
        got = (VC.fwd_kernel(c, E, K),)
    else:
        got = VC.select(c, E, K, L)
    assert got == kernels
    # the hand-out's length cap: 64 in all four, or the item size below it
    assert K["MAXK_FWD_STREAM"] == K["kCscGroupMax"] == K["kDenseGroupMax"] == 64


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@pytest.mark.gpu
@pytest.mark.parametrize("cid,chunk", PARAMS)
def test_handout_against_oracle(mk, cuda, cid, chunk):
    from test_parity_gpu import T
    op, k, _ = CASES[cid]
    p = prepared(k)
    g, ci = p["g"], p["ci"]
    rng = np.random.default_rng(k * 7 + chunk)
    rp, col, ev, civ = T(g.rp, cuda), T(g.col, cuda), T(g.ev, cuda), T(ci, cuda)
    for regime in ("unit", "mixed"):
        G = N.values(rng, (R, D), regime)
        cv = N.values(rng, ci.shape, regime)
        Gd, cvd = T(G, cuda), T(cv, cuda)
        for use_div in (True, False):
            gg = g if use_div else g._replace(div=None)
            div = T(g.div, cuda) if use_div else None
            what = f"{cid} chunk={chunk} {regime} row_div={use_div}"
            if op in ("fwd", "dense"):
                y = mk.spgemm_forward(rp, col, ev, cvd, civ, D, row_div=div, chunk=chunk)
            if op == "fwd_records":
                y = mk.spgemm_forward_records(rp, col, ev, mk.cbsr_records(cvd, civ, D), k, D,
                                              row_div=div, chunk=chunk)
            if op in ("fwd", "fwd_records", "dense"):
                N.within(y, N.fwd_ref(gg, cv, ci, D), N.bound_fwd(gg, cv, ci, D, n=p["nf"]),
                         what + " forward")
            if op in ("csc", "dense", "pick"):
                gs = mk.sspmm_backward(rp, col, ev, Gd, civ, row_div=div, chunk=chunk,
                                       mode="csc" if op == "csc" else "dense")
                N.within(gs, N.bwd_ref(gg, G, ci), N.bound_bwd(gg, G, ci, n=p["nb"]),
                         what + " backward")
