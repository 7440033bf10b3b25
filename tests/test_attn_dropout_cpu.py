"""CPU: the attention-dropout mask and its references (tests/attn_dropout_ref.py) -- the
generator's known answers, the drop count, the dropped forward and backward against torch
autograd of a dense float64 composition, the t identity -- and what of the three new C entries
can be checked without a device: the symbols, the signatures and the argument errors."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import attn_dropout_ref as DR
import gat_attention_bwd_ref as BR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols
from test_gat_attention_cpu import small_problem
from test_gat_attention_gpu import feat_grad_ref

DROP = "maxk_edge_dropout_heads"
FWD = "maxk_gat_attention_heads_dropout"
BWD = "maxk_gat_attention_heads_dropout_backward"
SYMBOLS = (DROP, FWD, FWD + "_workspace_size", BWD, BWD + "_workspace_size")


# ------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(w) for w in DR.philox4x32_10(counter, key))
    assert got == want, [hex(w) for w in got]


def test_threshold_and_scale():
    assert DR.threshold(0.0) == 0 and DR.threshold(0.5) == 1 << 31
    assert DR.threshold(np.nextafter(np.float32(1), np.float32(0))) == (1 << 32) - (1 << 8)
    assert DR.scale(0.0) == 1 and DR.scale(0.5) == 2
    assert DR.scale(0.6) == np.float32(1.0 / (1.0 - float(np.float32(0.6))))
    assert not DR.dropped(8, 100, 0.0, 7).any()


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_drop_count(p):
    """seed 12345, H = 8, E = 131072: the number of dropped pairs within 4 sigma of
    H E thr / 2^32, sigma^2 = H E p (1 - p).  A fixed seed: a deterministic test."""
    H, E = 8, 131072
    n = int(DR.dropped(H, E, p, 12345).sum())
    mean = H * E * DR.threshold(p) / 2.0 ** 32
    sigma = math.sqrt(H * E * p * (1 - p))
    print(f"\np {p}: {n} dropped, {(n - mean) / sigma:+.2f} sigma")
    assert abs(n - mean) <= 4 * sigma
    d = DR.mask(H, E, p, 12345)
    assert set(np.unique(d)) == {0.0, float(DR.scale(p))}


def test_masks_of_seeds_and_heads_differ():
    H, E = 8, 4096
    a, b = DR.dropped(H, E, 0.5, 1), DR.dropped(H, E, 0.5, 2)
    assert (a != b).mean() > 0.4
    assert (DR.dropped(H, E, 0.5, 1 << 32) != a).mean() > 0.4  # the high key word enters
    for h in range(H):
        for h2 in range(h):
            assert (a[h] != a[h2]).mean() > 0.4, (h, h2)
    # nothing but (seed, head, edge): fewer heads or edges are a prefix
    assert np.array_equal(DR.dropped(3, 100, 0.5, 1), a[:3, :100])


# ------------------------------------------------------------------------------- the formulas
def dense_dropped(g, ci, cv, s_dst, s_src, D, slope, G, d):
    """out and (grad s_dst, grad s_src, grad cv) of sum(out * G) in float64 torch, dense over the
    adjacency, the same d multiplied into the masked softmax."""
    R_, C = g.R, g.C
    rows = torch.from_numpy(np.repeat(np.arange(R_), np.diff(g.rp)))
    cols = torch.from_numpy(g.col.astype(np.int64))
    A = torch.zeros(R_, C, dtype=torch.float64)
    A[rows, cols] = 1.0
    Dm = torch.zeros(d.shape[0], R_, C, dtype=torch.float64)
    Dm[:, rows, cols] = torch.from_numpy(d)
    v = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    X = torch.zeros(C, 256, dtype=torch.float64).index_put(
        (torch.arange(C)[:, None].expand(-1, ci.shape[1]), torch.from_numpy(ci.astype(np.int64))),
        v, accumulate=True)[:, :D]
    sd = torch.from_numpy(s_dst.astype(np.float64)).requires_grad_(True)
    ss = torch.from_numpy(s_src.astype(np.float64)).requires_grad_(True)
    e = torch.nn.functional.leaky_relu(sd[:, :, None] + ss[:, None, :], slope)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 2) * A
    out = (alpha * Dm) @ X
    grads = torch.autograd.grad(out, [sd, ss, v], torch.from_numpy(G.astype(np.float64)))
    return out.detach().numpy(), [t.numpy() for t in grads]


@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_reference_agrees_with_dense_torch_autograd(slope, p):
    g, ci, cv, s_dst, s_src, D = small_problem()
    H = s_dst.shape[0]
    G = np.random.default_rng(2901).standard_normal((H, g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    ad, a, d = DR.attention(g.rp, g.col, s_dst, s_src, slope, cv, ci, D, n, p, 77)
    assert (d == 0).any() and (d > 0).any()
    b = DR.backward(g, a, ad, d, cv, ci, G, slope, D, BR.rounded_out_err(ad), feat_grad_ref)
    out, want = dense_dropped(g, ci, cv, s_dst, s_src, D, slope, G, d)
    assert np.abs(ad.out - out).max() <= 1e-12 * max(1.0, np.abs(out).max())
    for name, got, ref in (("s_dst", b.g_dst, want[0]), ("s_src", b.g_src, want[1]),
                           ("cbsr", b.g_cbsr, want[2])):
        err = np.abs(got - ref).max()
        assert got.shape == ref.shape and err <= 1e-12 * max(1.0, np.abs(ref).max()), (name, err)
    # the statistics are the undropped softmax's
    assert ad.m is a.m and ad.z is a.z
    # the t identity: sum_e alpha d ga == out . grad_out, to float64 rounding
    te = np.stack([np.bincount(a.heads[h].rows, a.w[h] * b.ga[h], minlength=g.R)
                   for h in range(H)])
    assert np.abs(te - b.t).max() <= 1e-12 * max(1.0, np.abs(b.t).max())
    # the rebuilt backward's reference is the same numbers
    st = DR.rebuilt_backward(g, a, d, BR.edge_grads(g, cv, ci, G), slope)
    assert np.abs(st.g_dst - b.g_dst).max() <= 1e-12 * max(1.0, np.abs(b.g_dst).max())
    assert np.abs(st.g_src - b.g_src).max() <= 1e-12 * max(1.0, np.abs(b.g_src).max())
    # structure: bounds are finite and non-negative, 0 exactly where nothing is added
    for ref, bound in ((ad.out, ad.out_bound), (b.g_dst, b.g_dst_bound), (b.g_src, b.g_src_bound),
                       (b.g_cbsr, b.g_cbsr_bound)):
        assert np.isfinite(bound).all() and (bound >= 0).all() and (ref[bound == 0] == 0).all()
    assert (ad.out_bound[:, n == 0] == 0).all()


def test_rounded_reference_is_inside_its_bounds():
    g, ci, cv, s_dst, s_src, D = small_problem()
    G = np.random.default_rng(2902).standard_normal((s_dst.shape[0], g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    ad, a, d = DR.attention(g.rp, g.col, s_dst, s_src, 0.2, cv, ci, D, n, 0.5, 5)
    for out_err in (BR.rounded_out_err(ad), ad.out_bound):
        b = DR.backward(g, a, ad, d, cv, ci, G, 0.2, D, out_err, feat_grad_ref)
        for ref, bound in ((ad.out, ad.out_bound), (b.g_dst, b.g_dst_bound),
                           (b.g_src, b.g_src_bound), (b.g_cbsr, b.g_cbsr_bound)):
            assert N.within(ref.astype(np.float32), ref, bound, "rounded") <= 0.5


def test_dropping_does_not_shield():
    """0 * NaN and 0 * Inf are NaN: a dropped edge's Inf value reaches the output."""
    g, ci, cv, s_dst, s_src, D = small_problem()
    n = N.count_fwd(g, ci, D)
    d = DR.mask(s_dst.shape[0], g.col.size, 0.5, 77)
    e = int(np.flatnonzero(d[0] == 0)[0])
    cv = cv.copy()
    cv[g.col[e], 0] = np.inf
    ad, _, _ = DR.attention(g.rp, g.col, s_dst, s_src, 0.2, cv, ci, D, n, 0.5, 77)
    r = np.repeat(np.arange(g.R), np.diff(g.rp))[e]
    assert np.isnan(ad.out[0, r, ci[g.col[e], 0]])


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz, u64 = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                                 ctypes.c_size_t, ctypes.c_uint64)
    assert _capi.SIGNATURES[DROP] == (ctypes.c_int, [p, p, i32, i64, f32, u64, p])
    assert _capi.SIGNATURES[FWD] == (ctypes.c_int, [p] * 4 + [f32] + [p] * 5 + [i64] * 3
                                     + [i32] * 4 + [f32, u64, p, sz, p])
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 6 + [f32] + [p] * 9 + [i64] * 3
                                     + [i32] * 4 + [f32, u64, p, sz, p])
    for s in (FWD, BWD):
        assert _capi.SIGNATURES[s + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 4)
    import maxk_cuda_kernels as mk
    assert callable(mk.edge_dropout_heads) and "edge_dropout_heads" in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced
OK = (10, 10, 5, 64, 8, 3, 0)  # rows, cols, e, D, k, H, chunk


def call_fwd(L, p, seed=1, shape=OK, ws_bytes=1 << 42, **named):
    names = "row_ptr col_idx s_dst s_src cbsr_val cbsr_idx out row_max row_sum".split()
    a = {n: named.get(n, P) for n in names}
    return L.maxk_gat_attention_heads_dropout(
        a["row_ptr"], a["col_idx"], a["s_dst"], a["s_src"], 0.2, a["cbsr_val"], a["cbsr_idx"],
        a["out"], a["row_max"], a["row_sum"], *shape, p, seed, P, ws_bytes, None)


def call_bwd(L, p, seed=1, shape=OK, ws_bytes=1 << 42, **named):
    names = ("row_ptr col_idx col_ptr csc_eid s_dst s_src cbsr_val cbsr_idx out row_max row_sum "
             "grad_out grad_s_dst grad_s_src grad_cbsr").split()
    a = {n: named.get(n, P) for n in names}
    return L.maxk_gat_attention_heads_dropout_backward(
        a["row_ptr"], a["col_idx"], a["col_ptr"], a["csc_eid"], a["s_dst"], a["s_src"], 0.2,
        a["cbsr_val"], a["cbsr_idx"], a["out"], a["row_max"], a["row_sum"], a["grad_out"],
        a["grad_s_dst"], a["grad_s_src"], a["grad_cbsr"], *shape, p, seed, P, ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    for p in (-0.1, 1.0, 1.5, math.nan, math.inf):
        for rc in (L.maxk_edge_dropout_heads(P, P, 3, 5, p, 1, None), call_fwd(L, p),
                   call_bwd(L, p)):
            assert rc == -1, p
            assert b"p must be in [0, 1)" in L.maxk_last_error()
    for p in (0.0, 0.5):  # p == 0 takes the entry without dropout's checks, p > 0 the same ones
        for H in (0, 9):
            assert L.maxk_edge_dropout_heads(P, P, H, 5, p, 1, None) == -1
            assert b"num_heads must be in [1,8]" in L.maxk_last_error()
            for call in (call_fwd, call_bwd):
                assert call(L, p, shape=OK[:5] + (H, 0)) == -1
                assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert L.maxk_edge_dropout_heads(P, P, 3, -1, p, 1, None) == -1
        assert b"num_e" in L.maxk_last_error()
        for w, out in ((None, P), (P, None)):
            assert L.maxk_edge_dropout_heads(w, out, 3, 5, p, 1, None) == -1
            assert b"NULL" in L.maxk_last_error()
        assert L.maxk_edge_dropout_heads(ctypes.c_void_p(4098), P, 3, 5, p, 1, None) == -1
        assert b"4-B aligned" in L.maxk_last_error()
        assert L.maxk_edge_dropout_heads(None, None, 3, 0, p, 1, None) == 0  # no edge: nothing
        for n in "row_ptr col_idx s_dst s_src cbsr_val cbsr_idx out row_max row_sum".split():
            assert call_fwd(L, p, **{n: None}) == -1, n
            msg = L.maxk_last_error()
            assert n.encode() in msg and b"NULL" in msg, (n, msg)
        for n in ("row_ptr col_idx col_ptr csc_eid s_dst s_src cbsr_val cbsr_idx out row_max "
                  "row_sum grad_out grad_s_dst grad_s_src grad_cbsr").split():
            assert call_bwd(L, p, **{n: None}) == -1, n
            msg = L.maxk_last_error()
            assert n.encode() in msg and b"NULL" in msg, (n, msg)
        for call in (call_fwd, call_bwd):
            assert call(L, p, ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()
    # the size queries are those of the entries without dropout
    for shape in (OK, (1000, 900, 5000, 256, 96, 8, 64)):
        assert L.maxk_gat_attention_heads_dropout_workspace_size(*shape) == \
            L.maxk_gat_attention_heads_workspace_size(*shape) > 0
        assert L.maxk_gat_attention_heads_dropout_backward_workspace_size(*shape) == \
            L.maxk_gat_attention_heads_backward_workspace_size(*shape) > 0


def test_binding_checks_rate_and_seed_before_any_tensor_work():
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    for p in (-0.1, 1.0, math.nan):
        with pytest.raises(RuntimeError, match="dropout must be in"):
            mk._dropout_args(p, 0)
        with pytest.raises(ValueError, match="attn_drop must be in"):
            ML.MaxKMultiHeadGATConv(4, 3, 2, attn_drop=p)
        with pytest.raises(ValueError, match="attn_drop must be in"):
            ML.MaxKGATConv(4, 3, attn_drop=p)
    for seed in (-1, 1 << 64):
        with pytest.raises(RuntimeError, match="seed must be in"):
            mk._dropout_args(0.5, seed)
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        mk.edge_dropout_heads(torch.zeros(2, 3), 0.5, 1)
    # a fresh seed per call from torch's default CPU generator, reproducible under manual_seed
    torch.manual_seed(3)
    a = [ML.attn_seed_of(None) for _ in range(3)]
    torch.manual_seed(3)
    assert [ML.attn_seed_of(None) for _ in range(3)] == a and len(set(a)) == 3
    assert all(0 <= s < 1 << 63 for s in a) and ML.attn_seed_of(11) == 11
