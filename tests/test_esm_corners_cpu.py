"""CPU: the corner graph of test_edge_softmax_corners_gpu.py holds the corners it is built for,
and the census that says so agrees with csrc/token_items.h.

tests/esm_corner_graph.py's census restates the cut-at-the-end rule on the tokens;
tests/esm_census.cpp (a stand-alone program that includes the header alone, built with the ROCm
install's host compiler like partition_check.cpp) walks the same pointer arrays with the header's
cont_piece / row_owned / row_piece, the way the edge softmax kernels do.  Both must list the same
pieces, item by item.  The corner classes are conditions on the inputs: over the item sizes the
GPU test runs, the row side (the corner graph's row pointer) and the column side (the CSC pointer
of its transpose) must each contain every one.  No kernel is launched.
"""
import subprocess

import numpy as np
import pytest

import esm_corner_graph as EG
from test_partition_cpu import CSRC, ROOT, host_compiler

SRC = f"{ROOT}/tests/esm_census.cpp"
KIND = {"W": EG.WHOLE, "T": EG.TAIL, "H": EG.HEAD}


def pointers():
    """name -> pointer array: both sides of both graphs, and the degenerate shapes."""
    rp, col = EG.corner_csr()
    trp, tcol = EG.corner_transpose()
    out = {"corner rows": rp, "corner columns": EG.csc_pointer(col, EG.NUM_COLS),
           "transpose rows": trp, "transpose columns": EG.csc_pointer(tcol, EG.NUM_ROWS)}
    for name, (drp, dcol, C) in EG.degenerate().items():
        out[name + " rows"] = drp
        out[name + " columns"] = EG.csc_pointer(dcol, C)
    return out


def test_graph_is_the_listed_one():
    rp, col = EG.corner_csr()
    deg = np.diff(rp)
    assert np.array_equal(deg, EG.DEGREES) and rp[-1] == col.size == 4553 and deg.size == 32
    assert deg[0] == 0 and (deg[13:15] == 0).all() and (deg[-3:] == 0).all()
    assert deg[EG.HUB_ROW] > 3 * 513
    assert col.min() >= 0 and col.max() < EG.NUM_COLS and not (col == EG.UNREAD).any()
    for r in range(deg.size):  # drawn without replacement, sorted
        assert (np.diff(col[rp[r]:rp[r + 1]]) > 0).all()
    trp, tcol = EG.corner_transpose()
    assert trp.size == EG.NUM_COLS + 1 and trp[-1] == col.size
    assert np.array_equal(EG.csc_pointer(tcol, EG.NUM_ROWS), rp), "the transpose's CSC pointer"
    assert np.array_equal(EG.csc_pointer(col, EG.NUM_COLS), trp)
    assert trp[EG.UNREAD + 1] == trp[EG.UNREAD]
    # the same edges
    rows = np.repeat(np.arange(32), deg)
    trows = np.repeat(np.arange(EG.NUM_COLS), np.diff(trp))
    assert set(zip(rows.tolist(), col.tolist())) == set(zip(tcol.tolist(), trows.tolist()))


@pytest.mark.parametrize("side", ["rows", "columns"])
def test_every_corner_class_is_present(side):
    if side == "rows":
        ptr = EG.corner_csr()[0]
    else:
        ptr = EG.csc_pointer(EG.corner_transpose()[1], EG.NUM_ROWS)
    found = {chunk: EG.corner_classes(ptr, chunk) for chunk in EG.CHUNKS}
    for chunk, f in found.items():
        print(chunk, sorted(f))
    missing = EG.ALL_CLASSES - set().union(*found.values())
    assert not missing, missing
    # where the classes that name a size must lie
    assert "row in as many pieces as edges" in found[1]
    assert "head piece of 512: an item inside one row" in found[512]
    assert "head piece of 513: an item inside one row" in found[513]


def test_last_item_is_clipped_at_the_token_total():
    """In "only the last row" the last item of 7 tokens ends at the token total, inside the
    only row that has edges."""
    rp, _, _ = EG.degenerate()["only the last row"]
    cs = EG.census(rp, 7)
    assert cs.total % 7 != 0 and cs.item.max() == cs.n_items - 1
    assert (np.diff(rp)[:-1] == 0).all() and np.diff(rp)[-1] > 0


def test_census_covers_every_token_once():
    """Each edge in exactly one piece, pieces inside their item's tokens, each row owned once."""
    for name, ptr in pointers().items():
        for chunk in EG.CHUNKS:
            c = EG.census(ptr, chunk)
            seen = np.zeros(int(ptr[-1]), np.int64)
            for sb, se in zip(c.sb, c.se):
                seen[sb:se] += 1
            assert (seen == 1).all(), (name, chunk)
            ln = c.se - c.sb
            has = ln > 0
            assert (c.sb[has] + c.row[has] + 1 >= c.item[has] * chunk).all()
            assert (c.se[has] + c.row[has] < (c.item[has] + 1) * chunk).all()
            assert c.item.max() < c.n_items and ln.max(initial=0) <= chunk
            owned = np.bincount(c.row[c.kind != EG.HEAD], minlength=c.deg.size)
            assert (owned == 1).all(), (name, chunk)


def test_census_agrees_with_the_header(tmp_path):
    exe = str(tmp_path / "esm_census")
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           f"-I{CSRC}", SRC, "-o", exe])
    n_pieces = 0
    for name, ptr in pointers().items():
        f = tmp_path / "ptr.txt"
        np.savetxt(f, np.asarray(ptr), fmt="%d")
        r = subprocess.run([exe, str(f)] + [str(c) for c in EG.CHUNKS], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        got, items = {}, {}
        for line in r.stdout.splitlines():
            t = line.split()
            if t[0] == "items":
                items[int(t[1])] = int(t[2])
            else:
                got.setdefault(int(t[0]), set()).add(
                    (int(t[1]), KIND[t[2]], int(t[3]), int(t[4]), int(t[5])))
        for chunk in EG.CHUNKS:
            c = EG.census(ptr, chunk)
            want = set(zip(c.item.tolist(), c.kind.tolist(), c.row.tolist(), c.sb.tolist(),
                           c.se.tolist()))
            assert len(want) == c.row.size
            assert items[chunk] == c.n_items, (name, chunk)
            assert got.get(chunk, set()) == want, (
                name, chunk, sorted(got.get(chunk, set()) ^ want)[:6])
            n_pieces += len(want)
    assert n_pieces > 20000
