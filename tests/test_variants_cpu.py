"""CPU guard of the variant cases (tests/variant_cases.py): each case's graph is rebuilt, the
statistics its launch rule reads are recomputed, and the rule -- restated in Python over the
constants parsed from csrc/ and the library's public rule functions -- must still select the
kernels the case names.  A retune that moves a threshold (kFwdSparseDegree, MAXK_CSC_GROUP_DEG,
kCscStage, kWave, the LDS fit of the pull ...) fails here instead of silently un-reaching a
variant that test_variants_gpu.py was written to reach.
"""
import functools
import re

import numpy as np
import pytest

import variant_cases as VC

IDS = [c.id for c in VC.CASES]


@pytest.fixture(scope="module")
def L():
    from maxk_cuda_kernels import _capi
    return _capi.load()


@functools.lru_cache(maxsize=None)
def K():
    return VC.constants()


def test_constants_parsed():
    """Every constant the rules read is found in the sources, with the values the case table
    was written for (a changed value is a retune: revisit the table)."""
    k = K()
    missing = [n for n in VC.REQUIRED if n not in k]
    assert not missing, missing
    assert k["kWave"] == 64
    assert k["kFwdSparseDegree"] == 128
    assert k["MAXK_CSC_GROUP_DEG"] == 16
    assert k["kCscStage"] == 2048
    assert k["kInfinityCacheBytes"] == 256 << 20
    assert k["kPullLdsBytes"] == 160 * 1024


@pytest.mark.parametrize("cid", IDS)
def test_case_selects_its_kernels(L, cid):
    c = VC.BY_ID[cid]
    k = K()
    if c.op == "topk":
        assert VC.select(c, 0, k, L) == c.kernels
        return
    rp, col = VC.build_csr(c)
    s = VC.stats(c, rp)
    deg = np.diff(rp)
    assert deg[0] == c.hub == deg.max() and deg[1] == 0, "hub row 0, empty row 1"
    assert int(col.max()) < c.C and not (col == VC.unread_column(c)).any()
    if c.chunk:
        assert c.hub > c.chunk, "the hub row is split over items"
    assert VC.select(c, s["E"], k, L) == c.kernels, s
    # the forward's output stays below the Infinity Cache: plain stores (spgemm_fwd.hip:896)
    assert c.R * c.D * 4 <= k["kInfinityCacheBytes"]
    if c.family == "push":
        # a row whose length is no multiple of the batch (64 / LR) * U
        lr, u = (int(x) for x in re.match(r"sspmm_bwd_kernel<(\d+), (\d+),", c.kernels[0]).groups())
        batch = k["kWave"] // lr * u
        assert (deg[2:] % batch != 0).any()
    if c.C >= 1 << 24:
        assert int(col.max()) == c.C - 1 and (col >= 1 << 24).any()
        # no buffer larger than the same one of test_tables_past_2_24_columns at k = 32
        what = {"csc": "csc", "wide_fwd": "fwd", "wide_eg": "eg"}[c.op]
        mine, theirs = VC.wide_bytes(c.k, what), VC.wide_bytes(32, "fwd")
        assert all(mine[b] <= theirs[b] for b in mine), (mine, theirs)


def test_public_rules_agree(L):
    """The library's own rule functions give what the table assumes: the bucket shifts of the
    pull cases, the dense route of the dense ones, and modes a caller can ask for."""
    assert L.maxk_bucket_shift(17) == 10 and L.maxk_pull_shift(17) == 10
    assert L.maxk_bucket_shift(18) == 9 and L.maxk_pull_shift(18) == 9
    for c in VC.CASES:
        if c.op == "pull" and "shift" in c.opts:
            # pull_impl accepts a plan's shift in [4, max(bucket shift, pull shift)]
            assert 4 <= c.opts["shift"] <= max(L.maxk_bucket_shift(c.k), L.maxk_pull_shift(c.k))
            assert L.maxk_pull_slices(c.R, c.C, c.D, c.k) >= 1
        if c.op == "dense":
            assert L.maxk_dense_route(c.D, c.k) == 1
            rp, _ = VC.build_csr(c)
            assert L.maxk_backward_mode_auto(c.R, c.C, int(rp[-1]), c.D, c.k, -1.0) == 6  # dense
        if c.op == "wide_fwd":
            rp, _ = VC.build_csr(c)
            assert L.maxk_records_ok(c.R, c.C, int(rp[-1]), c.D, c.k) == 0
            assert L.maxk_dense_route(c.D, c.k) == 0


def test_annotations_are_patterns():
    """WIDE and NOT_LAUNCHABLE name no kernel a case reaches."""
    reached = {kern for c in VC.CASES for kern in c.kernels}
    for pat in list(VC.WIDE) + list(VC.NOT_LAUNCHABLE):
        assert not [n for n in reached if re.fullmatch(pat, n)], pat
