"""The case table of test_variants_gpu.py and test_variants_cpu.py (a helper, like numerics.py).

The launch sites of libmaxk_hip.so pick a template instantiation from run-time statistics of
the call (average degree, num_cols >= 2^24, k / parts against the LDS, D, alignment).  Each
Case below is the smallest graph that makes one launch site pick an instantiation no other
small test reaches (profiles/r08/variant_reach/before.md, written by tools/variant_reach.py),
and names the kernels its call must launch.  select() restates the host rules in Python over
the constants parsed from csrc/ and the library's public rule functions: the CPU guard
recomputes every case's statistics and compares select() with the names in the table, so a
retune that moves a threshold fails there instead of silently un-reaching a variant; the GPU
file runs the case against the fp64 oracle.

Every graph is rectangular (R rows x C columns): the degree rules read E / R or E / C, so a
few dozen rows of the wanted length are enough.  Row 0 is a hub row (`hub` edges, split over
items by the case's explicit chunk), row 1 is empty, the others draw their length uniformly
from [dlo, dhi], so row lengths are no multiple of a batch; no edge reads column C // 3.

The alignment-selected kernels need no case: before.md shows pull_sel_kernel beside
pull_sel4_kernel and cbsr_pack_kernel beside cbsr_pack4_kernel (the forward's fall-back from the
dense route included) launched by the existing alignment tests of test_parity_gpu.py, and the
edge gradient's scalar staging is a run-time flag of one instantiation, not a template.

WIDE and NOT_LAUNCHABLE annotate the instantiations no small test can or should reach
(regular expressions over the names tools/variant_reach.py prints).
"""
import glob
import os
import re
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgemm-prunning_amd", "csrc")

Case = namedtuple("Case", "id family op k D R C dlo dhi hub chunk opts kernels rule")

WIDE_COLS = (1 << 24) + 4099  # test_parity_gpu.py::test_tables_past_2_24_columns' column space
# kernel modes of sspmm_push.hip:17
X4, X4W, X4S = 2, 3, 4


# ------------------------------------------------------------------------------- constants
def _cexpr(text):
    text = re.sub(r"(\d)(?:ull|ULL|ll|LL|u|U)\b", r"\1", text)
    if not re.fullmatch(r"[\d\s*+\-<>()/]+", text):
        raise ValueError(f"not a constant expression: {text!r}")
    return int(eval(text, {"__builtins__": {}}))  # digits and operators only (checked above)


def constants():
    """The constants the launch rules read, parsed from the sources: every `constexpr <int
    type> kName = <expr>;` and every default `#define MAXK_NAME <int>` of csrc/."""
    K = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read()
        for name, expr in re.findall(
                r"constexpr\s+(?:int|int64_t|size_t|unsigned)\s+(k[A-Z]\w*)\s*=\s*([^;]+);", src):
            try:
                K.setdefault(name, _cexpr(expr.split("//")[0].strip()))
            except ValueError:
                pass  # derived from other names: not one the rules below read
        for name, val in re.findall(r"#ifndef\s+(MAXK_\w+)[^\n]*\n(?:\s*//[^\n]*\n)*#define\s+\1\s+(-?\d+)\b", src):
            K.setdefault(name, int(val))
    return K


REQUIRED = ("kWave", "kFwdSparseDegree", "kCscStage", "kInfinityCacheBytes", "kPullLdsBytes",
            "kBucketAccDoubles", "MAXK_CSC_GROUP_DEG", "MAXK_CSC_GROUP_U", "MAXK_DENSE_U",
            "MAXK_DENSE_DMAX", "MAXK_PULL_QU", "MAXK_PULL_U", "MAXK_PULL_VPL8", "MAXK_BSORT_U",
            "MAXK_BUCKET_U", "MAXK_FWD_U", "MAXK_EGRAD_U", "MAXK_TOPK_ROWS4_KMAX",
            "MAXK_BWD_X4", "MAXK_X4_U", "MAXK_SUM_U", "MAXK_PULL_Q")


# ------------------------------------------------------------------------------- graphs
def _rng(c):
    return np.random.default_rng(zlib.crc32(c.id.encode()))


def build_csr(c):
    """(row_ptr int32, col int32) of the case: hub row 0, empty row 1, the rest in [dlo, dhi]."""
    rng = _rng(c)
    deg = rng.integers(c.dlo, c.dhi + 1, c.R)
    deg[0], deg[1] = c.hub, 0
    assert deg.max() <= c.C - 1
    u = unread_column(c)
    rows = [np.sort(rng.choice(c.C - 1, int(d), replace=False)) for d in deg]
    rows = [r + (r >= u) for r in rows]  # no edge reads column u
    if c.C >= 1 << 24:  # the table's end is read
        rows[2] = np.unique(np.concatenate([rows[2], c.C - 1 - np.arange(3)]))
    rp = np.zeros(c.R + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return rp.astype(np.int32), np.concatenate(rows).astype(np.int32)


def unread_column(c):
    """A column no edge reads: its gradient row has no addend and must be exactly zero."""
    return c.C // 3


def stats(c, rp):
    E = int(rp[-1])
    return {"E": E, "out_degree": E // c.R, "in_degree": E // c.C}


# ------------------------------------------------------------------------------- the rules
def lanes_per_edge(k, wave):
    """common.h lanes_per_edge: the next power of two >= k, capped at a wave."""
    g = 1
    while g < k and g < wave:
        g <<= 1
    return g


def pick_depth(E, rows, per_step, lo, hi):
    """sspmm_push.hip pick_depth: the largest U in [lo, hi] with per_step * U <= E / rows."""
    avg = E // rows if rows > 0 else 0
    u = lo
    while u < hi and per_step * u * 2 <= avg:
        u <<= 1
    return u


def _b(x):
    return "true" if x else "false"


def push_kernel(c, E, K):
    """launch_push<kStore> (sspmm_push.hip:562-603), k % 4 == 0: LR = lanes_per_edge(k / 4),
    U from pick_depth(E, rows, kWave / LR, 4, 16); the mode is the selector stream (edge_sel
    given), the wide table (num_cols >= 2^24, depth 8 only) or the table."""
    assert c.k % 4 == 0 and K["MAXK_BWD_X4"] == 1 and K["MAXK_X4_U"] == 0
    lr = lanes_per_edge(c.k // 4, K["kWave"])
    u = pick_depth(E, c.R, K["kWave"] // lr, 4, 16)
    mode = X4S if c.opts.get("esel") else X4W if c.C >= 1 << 24 else X4
    depth = 8 if mode == X4W else 4 if u <= 4 else 8 if u <= 8 else 16
    return f"sspmm_bwd_kernel<{lr}, {depth}, {mode}>"


def csc_sum_kernel(c, E, K):
    """csc_impl (sspmm_push.hip:701-747): staged at chunk <= kCscStage, nt at k % 32 == 0; a
    power-of-two k >= 4 sums 16 B per lane, in lane groups per destination (k in [16, 64],
    staged, E < MAXK_CSC_GROUP_DEG * num_cols) or at depth pick_depth(E, num_cols, kWave /
    (k / 4), 2, 8); any other k one l per lane at depth 4."""
    assert c.chunk > 0 and K["MAXK_SUM_U"] == 0
    k = c.k
    staged = c.chunk <= K["kCscStage"]
    nt = k % 32 == 0
    vec = k >= 4 and k & (k - 1) == 0
    if staged and vec and 16 <= k <= 64 and E < K["MAXK_CSC_GROUP_DEG"] * c.C:
        return f"csc_sum_kernel<true, 64, {K['MAXK_CSC_GROUP_U']}, true, true, {_b(nt)}>"
    if vec:
        u = pick_depth(E, c.C, K["kWave"] // (k // 4), 2, 8)
        u = 2 if u <= 2 else 4 if u <= 4 else 8
        return f"csc_sum_kernel<true, 64, {u}, {_b(staged)}, false, {_b(staged and nt)}>"
    return f"csc_sum_kernel<false, {lanes_per_edge(k, K['kWave'])}, 4, {_b(staged)}, false, false>"


def dense_lanes(D):
    """dense_route.hip dense_lanes: lanes of 4 columns covering D."""
    lr = 1
    while lr * 4 < D:
        lr <<= 1
    return lr


def pull_kernel(c, K, L):
    """pull_impl (sspmm_pull.hip:653-774): k % 4 == 0 takes pull_q_kernel with the fewest parts
    H whose k / H slots fit the LDS at the plan's bucket shift (pull_parts, :625), LR =
    lanes_per_edge(kp / 4), FULLD at D == 256; any other k pull_tile_kernel, one l per lane,
    its selectors in LDS when the padded accumulator and they fit kPullLdsBytes."""
    k, lds = c.k, K["kPullLdsBytes"]
    shift = c.opts.get("shift")
    shift = int(L.maxk_pull_shift(k)) if shift is None else shift
    assert 4 <= shift <= 15
    parts = 0
    if K["MAXK_PULL_Q"] and k % 4 == 0:
        H = 1
        while H <= k // 4 and k % (4 * H) == 0:
            if ((k // H) * 8 + k // H) << shift <= lds:
                parts = H
                break
            H *= 2
    if parts:
        kp = k // parts
        vpl = 4 if kp != 8 else K["MAXK_PULL_VPL8"] or (8 if parts == 1 else 4)
        lr = lanes_per_edge(kp // 4, K["kWave"]) if vpl == 4 else kp // vpl
        return f"pull_q_kernel<{lr}, {K['MAXK_PULL_QU']}, {_b(c.D == 256)}, {vpl}>"
    assert shift <= int(L.maxk_bucket_shift(k))  # pull_impl's check for the tile kernel
    sel_lds = (((k + 1) << shift) * 8 + (k << shift)) <= lds
    v4 = k % 4 == 0
    lr = lanes_per_edge(k // 4 if v4 else k, K["kWave"])
    return f"pull_tile_kernel<{lr}, {K['MAXK_PULL_U']}, {_b(sel_lds)}, {4 if v4 else 1}>"


def record_stride(k, num_cols):
    """cbsr_pack.h record_stride."""
    b = 6 * k
    if b <= 128:
        s = 16
        while s < b:
            s <<= 1
        return s
    s64 = (b + 63) // 64 * 64
    return s64 if s64 * num_cols <= 128 << 20 else (b + 127) // 128 * 128


def fwd_kernel(c, E, K):
    """fwd_layout / launch_fwd (spgemm_fwd.hip:733-796), no selector stream written: KG =
    max(lanes_per_edge(k), 16 on a graph of average degree < kFwdSparseDegree, else 8); deep on
    a dense graph, streaming rows on a sparse one at KG 16 / 32 and D % 4 == 0, both only with
    32-bit record offsets (num_cols < 2^24, table < 4 GiB); past them the WIDE walker."""
    sparse = E < K["kFwdSparseDegree"] * c.R
    kg = max(lanes_per_edge(c.k, K["kWave"]), 16 if sparse else 8)
    narrow = c.C < 1 << 24 and c.C * record_stride(c.k, c.C) < 1 << 32
    U = K["MAXK_FWD_U"]
    if narrow and sparse and 16 <= kg <= 32 and c.D % 4 == 0:
        return f"spgemm_fwd_kernel<{kg}, {U}, false, false, true>"
    if narrow and not sparse:
        return f"spgemm_fwd_kernel<{kg}, {2 * U}, false, false, false>"
    return f"spgemm_fwd_kernel<{kg}, {U}, {_b(not narrow)}, false, false>"


def edge_grad_kernel(c, K):
    """edge_grad_layout (edge_grad.hip:219-233): KG = max(lanes_per_edge(k), 8); WIDE past
    32-bit record offsets."""
    kg = max(lanes_per_edge(c.k, K["kWave"]), 8)
    wide = not (c.C < 1 << 24 and c.C * record_stride(c.k, c.C) < 1 << 32)
    return f"edge_grad_kernel<{kg}, {K['MAXK_EGRAD_U']}, {_b(wide)}>"


def topk_kernel(c, K):
    """topk_launch (topk_cbsr.hip:608-645): four rows per wave up to k = MAXK_TOPK_ROWS4_KMAX
    (J = 2 lane keys up to k = 32, else 4; VEC when D % 4 == 0 and x is aligned to four
    elements), one row per wave above."""
    t = "unsigned char" if c.opts["dtype"] == "u8" else "float"
    if c.k > K["MAXK_TOPK_ROWS4_KMAX"]:
        return f"topk_cbsr_kernel<{t}>"
    vec = c.D % 4 == 0 and not c.opts.get("offset")
    return f"topk_rows4_kernel<{t}, {_b(vec)}, {2 if c.k <= 32 else 4}>"


def select(c, E, K, L=None):
    """The variant-selected kernels the case's calls launch, by the rules above (L: the loaded
    library, for its public rule functions)."""
    wave = K["kWave"]
    if c.op == "csc":
        return (push_kernel(c, E, K), csc_sum_kernel(c, E, K))
    if c.op == "bsort":
        lr = lanes_per_edge(c.k // 4, wave)  # sspmm_bsort.hip:331, :399
        return (f"bsort_push_kernel<{lr}, {K['MAXK_BSORT_U']}, {_b(c.opts.get('esel'))}>",
                f"bucket_sum_kernel<{lr}, {K['MAXK_BUCKET_U']}>")
    if c.op == "dense":
        # forward_impl (spgemm_fwd.hip:850) takes the dense route where maxk_dense_route holds;
        # the backward (dense_route.hip:804) picks columns below k = D / 2, else selects rows
        assert L.maxk_dense_route(c.D, c.k) == 1 and c.D <= K["MAXK_DENSE_DMAX"]
        assert not (2 * c.k < c.D and c.k <= wave)
        lr, U = dense_lanes(c.D), K["MAXK_DENSE_U"]
        return (f"dense_rows_kernel<{lr}, {U}>", f"dense_select_rows_kernel<{lr}, {U}>")
    if c.op == "pull":
        return (pull_kernel(c, K, L),)
    if c.op == "wide_fwd":
        return (fwd_kernel(c, E, K),)
    if c.op == "wide_eg":
        return (edge_grad_kernel(c, K),)
    if c.op == "topk":
        return (topk_kernel(c, K),)
    raise ValueError(c.op)


# ------------------------------------------------------------------------------- the table
def _case(id, family, op, k, D, R, C, dlo, dhi, hub, chunk, kernels, rule, **opts):
    return Case(id, family, op, k, D, R, C, dlo, dhi, hub, chunk, opts, tuple(kernels), rule)


_PUSH = ("sspmm_push.hip:572-576 launch_push: LR = lanes_per_edge(k/4) = {lr}; U doubles from 4 "
         "while (64/LR)*U*2 <= E/rows, so U = {u} needs E/rows in {win}")
_SUM = "; sspmm_push.hip:721-744 csc_impl picks the phase-2 kernel"


def _push_cases():
    #    k    U   R    C     dlo   dhi   hub   chunk  window of E / rows   csc_sum kernel
    rows = [
        (4,   8,  48,  2048, 600,  660,  2000, 1500, "[512, 1024)", "true, 64, 2, true, false, false"),
        (4,   16, 48,  2048, 1040, 1100, 2000, 1500, "[1024, inf)", "true, 64, 2, true, false, false"),
        (8,   8,  48,  1024, 300,  340,  1000, 700,  "[256, 512)",  "true, 64, 2, true, false, false"),
        (8,   16, 48,  1024, 530,  570,  1000, 700,  "[512, inf)",  "true, 64, 2, true, false, false"),
        (16,  16, 48,  600,  270,  300,  590,  400,  "[256, inf)",  "true, 64, 2, true, false, false"),
        (32,  8,  64,  400,  70,   100,  390,  300,  "[64, 128)",   "true, 64, 4, true, true, true"),
        (32,  16, 64,  400,  135,  160,  390,  300,  "[128, inf)",  "true, 64, 2, true, false, true"),
        (64,  8,  64,  300,  36,   50,   290,  200,  "[32, 64)",    "true, 64, 4, true, true, true"),
        (64,  16, 64,  300,  70,   90,   290,  200,  "[64, inf)",   "true, 64, 4, true, false, true"),
        (128, 4,  100, 300,  3,    9,    290,  200,  "[0, 16)",     "true, 64, 2, true, false, true"),
        (128, 8,  100, 300,  17,   24,   290,  200,  "[16, 32)",    "true, 64, 2, true, false, true"),
        (128, 16, 100, 300,  34,   50,   290,  200,  "[32, inf)",   "true, 64, 4, true, false, true"),
        (256, 4,  200, 300,  1,    5,    290,  200,  "[0, 8)",      "true, 64, 2, true, false, true"),
        (256, 8,  200, 300,  8,    12,   290,  200,  "[8, 16)",     "true, 64, 4, true, false, true"),
        (256, 16, 200, 300,  17,   30,   290,  200,  "[16, inf)",   "true, 64, 8, true, false, true"),
    ]
    # the table form of these depths is reached by test_parity_gpu.py already: stream only
    stream_only = {(16, 16), (64, 16), (128, 4), (256, 8)}
    out = []
    for k, u, R, C, dlo, dhi, hub, chunk, win, ssum in rows:
        lr = lanes_per_edge(k // 4, 64)
        rule = _PUSH.format(lr=lr, u=u, win=win) + _SUM
        for esel, mode in ((False, X4), (True, X4S)):
            if not esel and (k, u) in stream_only:
                continue
            out.append(_case(f"push-k{k}-u{u}" + ("-esel" if esel else ""), "push", "csc", k, 256,
                             R, C, dlo, dhi, hub, chunk,
                             (f"sspmm_bwd_kernel<{lr}, {u}, {mode}>", f"csc_sum_kernel<{ssum}>"),
                             rule + (" (sspmm_push.hip:575: edge_sel given, kStoreX4S)" if esel else ""),
                             esel=esel))
    return out


CASES = _push_cases() + [
    _case("sum-k12-unstaged", "csc_sum", "csc", 12, 256, 48, 5000, 100, 140, 4990, 4096,
          ("sspmm_bwd_kernel<4, 8, 2>", "csc_sum_kernel<false, 16, 4, false, false, false>"),
          "sspmm_push.hip:704 staged = chunk <= kCscStage (2048): chunk 4096 reads csc_eid from "
          "global memory; :740-743 k = 12 is no power of two: one l per lane, KG = 16"),
    _case("sum-k16-u4", "csc_sum", "csc", 16, 256, 300, 64, 15, 25, 60, 40,
          ("sspmm_bwd_kernel<4, 4, 2>", "csc_sum_kernel<true, 64, 4, true, false, false>"),
          "sspmm_push.hip:727-737: k = 16 sums 16 rows per wave step, u = pick_depth(E, num_cols, "
          "16, 2, 8) = 4 needs E/num_cols in [64, 128); staged (chunk 40), no whole-line rows "
          "(k % 32 != 0); :721 not grouped: E >= MAXK_CSC_GROUP_DEG * num_cols"),
    _case("bsort-k128-esel", "bsort", "bsort", 128, 256, 100, 300, 17, 24, 290, 0,
          ("bsort_push_kernel<32, 2, true>", "bucket_sum_kernel<32, 8>"),
          "sspmm_bsort.hip:399-403: LR = lanes_per_edge(k/4) = 32 for k in [68, 128], ES = "
          "edge_sel given", esel=True),
    _case("dense-D16-k8", "dense", "dense", 8, 16, 150, 200, 5, 40, 190, 60,
          ("dense_rows_kernel<4, 4>", "dense_select_rows_kernel<4, 4>"),
          "dense_route.hip:688 LR = dense_lanes(D) = 4 for D in (8, 16]; :710 dense_route: "
          "D % 4 == 0, D <= 128, k % 4 == 0, 2k >= D; :804 2k >= D: rows selected, not picked"),
    _case("dense-D32-k16", "dense", "dense", 16, 32, 150, 200, 5, 40, 190, 60,
          ("dense_rows_kernel<8, 4>", "dense_select_rows_kernel<8, 4>"),
          "dense_route.hip:688 LR = dense_lanes(D) = 8 for D in (16, 32]; :710 dense_route; "
          ":804 2k >= D: rows selected, not picked"),
    _case("pull-k17", "pull_tile", "pull", 17, 256, 150, 1500, 5, 40, 1490, 0,
          ("pull_tile_kernel<32, 4, false, 1>",),
          "sspmm_pull.hip:760 k % 4 != 0: one l per lane, LR = lanes_per_edge(17) = 32; :712 at "
          "the default shift 10 (2^10 * 18 = kBucketAccDoubles) the padded accumulator plus the "
          "selectors, (9k + 8) << 10 = 164864 B, pass kPullLdsBytes: selectors read from global"),
    _case("pull-k18", "pull_tile", "pull", 18, 256, 150, 1500, 5, 40, 1490, 0,
          ("pull_tile_kernel<32, 4, true, 1>",),
          "sspmm_pull.hip:760 LR = lanes_per_edge(18) = 32; :712 at the default shift 9 the "
          "accumulator and selectors fit: selectors in LDS"),
    _case("pull-k128-D128-s4", "pull_q", "pull", 128, 128, 150, 300, 5, 40, 290, 0,
          ("pull_q_kernel<32, 2, false, 4>",),
          "sspmm_pull.hip:625 pull_parts(128, 4) = 1: 128 slots per destination fit the LDS in "
          "buckets of 2^4 (pull_plan(shift=4)); :742 LR = lanes_per_edge(128/4) = 32; :738 D < 256",
          shift=4, slices=3),
    _case("pull-k128-D256-s4", "pull_q", "pull", 128, 256, 150, 300, 5, 40, 290, 0,
          ("pull_q_kernel<32, 2, true, 4>",),
          "sspmm_pull.hip:625 pull_parts(128, 4) = 1; :742 LR = 32; :738 FULLD: D == 256",
          shift=4, slices=3),
    _case("pull-k132-D132-s4", "pull_q", "pull", 132, 132, 150, 300, 5, 40, 290, 0,
          ("pull_q_kernel<64, 2, false, 4>",),
          "sspmm_pull.hip:625 pull_parts(132, 4) = 1; :742 LR = lanes_per_edge(33) = 64; :738 "
          "D < 256", shift=4, slices=3),
    _case("pull-k256-s4", "pull_q", "pull", 256, 256, 150, 300, 5, 40, 290, 0,
          ("pull_q_kernel<64, 2, true, 4>",),
          "sspmm_pull.hip:625 pull_parts(256, 4) = 1; :742 LR = lanes_per_edge(64) = 64; :738 "
          "FULLD", shift=4, slices=3),
    # ---- tables past 2^24 columns: the lane groups whose buffers are no larger than those of
    # test_parity_gpu.py::test_tables_past_2_24_columns at k = 32 (k <= 32)
    _case("wide-csc-k4", "wide", "csc", 4, 256, 300, WIDE_COLS, 0, 40, 900, 50,
          ("sspmm_bwd_kernel<1, 8, 3>", "csc_sum_kernel<true, 64, 2, true, false, false>"),
          "sspmm_push.hip:573-576 num_cols >= 2^24: kStoreX4W, depth 8 only; LR = 1 at k = 4"),
    _case("wide-csc-k16", "wide", "csc", 16, 256, 300, WIDE_COLS, 0, 40, 900, 50,
          ("sspmm_bwd_kernel<4, 8, 3>", "csc_sum_kernel<true, 64, 4, true, true, false>"),
          "sspmm_push.hip:573-576 num_cols >= 2^24: kStoreX4W; LR = 4 at k = 16"),
    _case("wide-fwd-k8-dense", "wide", "wide_fwd", 8, 256, 40, WIDE_COLS, 150, 250, 900, 50,
          ("spgemm_fwd_kernel<8, 8, true, false, false>",),
          "spgemm_fwd.hip:48-52 KG = 8 needs k <= 8 on a graph of E >= kFwdSparseDegree * rows; "
          ":739-740 num_cols >= 2^24 is not narrow, so not deep; :792 the WIDE walker"),
    _case("wide-eg-k16", "wide", "wide_eg", 16, 256, 300, WIDE_COLS, 0, 40, 900, 64,
          ("edge_grad_kernel<16, 8, true>",),
          "edge_grad.hip:224-226 KG = lanes_per_edge(16) = 16, wide at num_cols >= 2^24"),
    _case("wide-eg-k32", "wide", "wide_eg", 32, 256, 300, WIDE_COLS, 0, 40, 900, 64,
          ("edge_grad_kernel<32, 8, true>",),
          "edge_grad.hip:224-226 KG = 32, wide at num_cols >= 2^24 (the record table also "
          "passes 4 GiB)"),
    # ---- top-k: R rows of D columns; C, the degrees and the chunk are unused
    _case("topk-u8-k40", "topk", "topk", 40, 256, 301, 0, 0, 0, 0, 0,
          ("topk_rows4_kernel<unsigned char, true, 4>",),
          "topk_cbsr.hip:618 k <= MAXK_TOPK_ROWS4_KMAX (48): four rows per wave; :632 k > 32: "
          "J = 4; :623 D % 4 == 0 and aligned: VEC", dtype="u8"),
    _case("topk-u8-k40-D254", "topk", "topk", 40, 254, 301, 0, 0, 0, 0, 0,
          ("topk_rows4_kernel<unsigned char, false, 4>",),
          "topk_cbsr.hip:623 D % 4 != 0: not VEC; :632 J = 4", dtype="u8"),
    _case("topk-u8-k56", "topk", "topk", 56, 256, 301, 0, 0, 0, 0, 0,
          ("topk_cbsr_kernel<unsigned char>",),
          "topk_cbsr.hip:618 k > MAXK_TOPK_ROWS4_KMAX: one row per wave", dtype="u8"),
    _case("topk-f32-k40-D101", "topk", "topk", 40, 101, 301, 0, 0, 0, 0, 0,
          ("topk_rows4_kernel<float, false, 4>",),
          "topk_cbsr.hip:623 D % 4 != 0: not VEC; :632 k in (32, 48]: J = 4", dtype="f32"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

#: Inf / NaN inputs (numerics.poison): one case per kernel family this file adds cases to
POISONED = ("push-k4-u16", "push-k8-u16-esel", "bsort-k128-esel", "pull-k256-s4")


def wide_bytes(k, what):
    """Bytes of the largest buffers a call past 2^24 columns holds at width k: the CBSR values
    or the gradient ([num_cols, k] fp32), the selectors, and (forward, edge gradient) the
    record table."""
    n = WIDE_COLS
    b = {"values": n * k * 4, "selectors": n * k}
    if what != "csc":
        b["records"] = n * record_stride(k, n)
    return b


# instantiations only a table past 2^24 columns selects, at a k whose buffers pass those of
# test_tables_past_2_24_columns at k = 32 (2 GiB of values, 4 GiB of records): bytes needed
WIDE = {
    r"sspmm_bwd_kernel<16, 8, 3>": sum(wide_bytes(36, "csc").values()),
    r"sspmm_bwd_kernel<32, 8, 3>": sum(wide_bytes(68, "csc").values()),
    r"spgemm_fwd_kernel<64, 8, true, false, false>": sum(wide_bytes(36, "fwd").values()),
    r"edge_grad_kernel<64, 8, true>": sum(wide_bytes(36, "eg").values()),
}

NOT_LAUNCHABLE = {
    r"sspmm_bwd_kernel<64, 8, 3>":
        "sspmm_bwd.h:35 num_cols * k < 2^31: LR = 64 needs k >= 132, the wide table num_cols >= 2^24",
    r"spgemm_fwd_kernel<64, 8, false, false, true>":
        "spgemm_fwd.hip:741 L.stream needs kg <= 32",
    r"spgemm_fwd_kernel<8, 8, false, false, false>":
        "spgemm_fwd.hip:50 KG = 8 needs a dense graph, which with 32-bit record offsets is deep "
        "(:740, U = 16) and without them WIDE (:792)",
    r"dense_rows_kernel<64, 4>":
        "dense_route.hip:711 the forward's dense route stops at D <= MAXK_DENSE_DMAX = 128: "
        "dense_lanes(D) <= 32",
    r"pick_rows_kernel<[12], 4>":
        "dense_route.hip:794 the dense backward needs k % 4 == 0: lanes_per_edge(k) >= 4",
    r"pull_q_kernel<4, 2, (true|false), 2>":
        "sspmm_pull.hip:724 two values per lane only with MAXK_PULL_VPL8 = 2 (default 0)",
    r"pull_tile_kernel<\d+, 4, (true|false), 4>":
        "sspmm_pull.hip:666-673 with MAXK_PULL_Q = 1 a k % 4 == 0 takes pull_q_kernel whenever "
        "four slots fit (shift <= 12), and a shift past maxk_bucket_shift(k) <= 11 is rejected",
    r"pull_tile_kernel<(1|2|4|8|16), 4, false, 1>":
        "sspmm_pull.hip:712 at shift <= maxk_bucket_shift(k) the accumulator and selectors pass "
        "kPullLdsBytes only for k > 8 with 2^shift * (k + 1) near kBucketAccDoubles: k = 17, 35",
}
