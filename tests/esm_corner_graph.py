"""The corner graph of test_esm_corners_cpu.py and test_edge_softmax_corners_gpu.py (a helper, like
handout_graph.py), and a census of the pieces a pointer array falls into under the cut-at-the-end
rule of csrc/token_items.h.

The graph: 32 rows whose degrees are DEGREES, in row order -- the lengths on either side of the
lane groups' 32 edges (kShort) and of the 512 a wave holds in registers (kRegPiece), a first row
without edges, two consecutive empty rows, trailing empty rows (the last item's hand-out runs into
num_rows) and one hub of 1700 edges, longer than three items of 513 tokens.  Columns are drawn
without replacement from NUM_COLS columns, UNREAD left out.  corner_transpose() is the same
graph transposed (NUM_COLS rows, 32 columns), so its CSC pointer array is the prefix sum of
DEGREES and the column sums of the GAT backward meet the same corners.  Nothing is written to
disk.

The census restates the token rule on the tokens themselves: row q's token is q + ptr[q], edge e
of row q is token e + q + 1, item i holds the tokens [i * chunk, (i + 1) * chunk), a row is owned
by the item holding its token, and an item walks exactly the edges whose tokens it holds.  A piece
is a maximal run of one row's edges inside one item:

    whole  the row's only piece, in its owner (a row without edges is a whole piece of length 0);
    tail   in the owner, the row going on into later items (of length 0 when the row's token is
           the owner's last: the owner holds none of it);
    head   in a later item than the owner.

test_esm_corners_cpu.py checks it against a walk by the header's own functions.
"""
import functools
from collections import namedtuple

import numpy as np

DEGREES = (0, 1, 2, 7, 8, 9, 31, 32, 33, 34, 63, 64, 65, 0, 0, 127, 128, 129, 511, 512, 513, 514,
           1, 1700, 3, 0, 32, 33, 1, 0, 0, 0)
NUM_ROWS = len(DEGREES)
HUB_ROW = DEGREES.index(1700)
NUM_COLS = 1710
UNREAD = 1234
#: the item sizes of the GPU test (0, the library's own rule, is added there)
CHUNKS = (1, 2, 7, 33, 64, 67, 512, 513, 4096)

Census = namedtuple("Census", "chunk n_items total row item sb se kind owner deg")
WHOLE, TAIL, HEAD = 0, 1, 2


def pointer(degrees):
    p = np.zeros(len(degrees) + 1, np.int64)
    np.cumsum(degrees, out=p[1:])
    return p


@functools.lru_cache(maxsize=None)
def corner_csr():
    """(row_ptr int32 [33], col int32 [E]): sorted distinct columns per row, never UNREAD."""
    rng = np.random.default_rng(1101)
    pool = np.delete(np.arange(NUM_COLS), UNREAD)
    col = [np.sort(rng.choice(pool, d, replace=False)) for d in DEGREES]
    return pointer(DEGREES).astype(np.int32), np.concatenate(col).astype(np.int32)


@functools.lru_cache(maxsize=None)
def corner_transpose():
    """(row_ptr int32 [NUM_COLS + 1], col int32 [E]) of the transpose: row c lists the rows of
    corner_csr() that read column c, in order."""
    rp, col = corner_csr()
    rows = np.repeat(np.arange(NUM_ROWS), np.diff(rp))
    order = np.lexsort((rows, col))
    return (pointer(np.bincount(col, minlength=NUM_COLS)).astype(np.int32),
            rows[order].astype(np.int32))


@functools.lru_cache(maxsize=None)
def degenerate():
    """name -> (row_ptr, col, num_cols): the shapes with one of everything."""
    rng = np.random.default_rng(1102)
    i32 = lambda a: np.asarray(a, np.int32)  # noqa: E731
    one_row = np.sort(rng.choice(640, 600, replace=False))
    return {
        "one row of 600": (i32([0, 600]), i32(one_row), 640),
        "600 rows of one": (i32(np.arange(601)), i32(rng.integers(0, 50, 600)), 50),
        "a single edge": (i32([0, 1]), i32([0]), 1),
        "one column, 300 duplicates": (i32(pointer([30] * 10)), i32(np.zeros(300)), 1),
        "only the last row": (i32(pointer([0] * 39 + [101])),
                              i32(np.sort(rng.choice(128, 101, replace=False))), 128),
    }


def csc_pointer(col, num_cols):
    """The pointer array the column sums walk: the CSC's."""
    return pointer(np.bincount(col, minlength=num_cols))


def census(ptr, chunk):
    """Every piece of the pointer array at items of `chunk` tokens, as parallel arrays (row,
    item, sb, se, kind), empty rows included; owner[q]: the item of row q's token."""
    ptr = np.asarray(ptr, np.int64)
    n = ptr.size - 1
    E = int(ptr[-1])
    deg = np.diff(ptr)
    total = n + E
    n_items = max(1, -(-total // chunk))
    owner = (np.arange(n) + ptr[:-1]) // chunk
    e_row = np.repeat(np.arange(n), deg)
    e_item = (np.arange(E) + e_row + 1) // chunk
    # a piece starts where the (row, item) of consecutive edges changes
    first = np.ones(E, bool)
    first[1:] = (e_row[1:] != e_row[:-1]) | (e_item[1:] != e_item[:-1])
    sb = np.flatnonzero(first)
    se = np.append(sb[1:], E)
    row, item = e_row[sb], e_item[sb]
    last_item = np.where(deg > 0, e_item[np.maximum(ptr[1:] - 1, 0)] if E else 0, owner)
    kind = np.where(item > owner[row], HEAD, np.where(last_item[row] > item, TAIL, WHOLE))
    # owned rows without an edge in their owner: empty rows (whole), and rows whose token is the
    # item's last (a tail of length 0)
    first_item = np.where(deg > 0, e_item[np.minimum(ptr[:-1], max(E - 1, 0))] if E else 0, owner)
    bare = np.flatnonzero((deg == 0) | (first_item > owner))
    row = np.concatenate([row, bare])
    item = np.concatenate([item, owner[bare]])
    sb = np.concatenate([sb, ptr[bare]])
    se = np.concatenate([se, ptr[bare]])
    kind = np.concatenate([kind, np.where(deg[bare] == 0, WHOLE, TAIL)])
    return Census(chunk, n_items, total, row, item, sb, se, kind, owner, deg)


def slots_per_row(ptr, chunk):
    """The number of slots the merge joins for each row: its pieces when it has more than one
    (a tail that holds no edge has no slot), else 0."""
    c = census(ptr, chunk)
    cut = (c.kind != WHOLE) & (c.se > c.sb)
    return np.bincount(c.row[cut], minlength=c.deg.size)


def corner_classes(ptr, chunk):
    """The names of the corner classes this (pointer array, item size) contains."""
    c = census(ptr, chunk)
    ln = c.se - c.sb
    whole, tail, head = c.kind == WHOLE, c.kind == TAIL, c.kind == HEAD
    d1 = np.minimum((c.item + 1) * chunk, c.total)
    found = set()
    for k in (32, 33, 512, 513):
        if (whole & (ln == k)).any():
            found.add(f"whole row of {k}")
    for k in (512, 513):
        if chunk == k and (head & (ln == k)).any():
            found.add(f"head piece of {k}: an item inside one row")
    for k in (32, 33):
        if (tail & (ln == k)).any():
            found.add(f"tail piece of {k}")
    # rows whose token is their item's last: the owner holds none of their edges
    none = np.zeros(c.deg.size, bool)
    none[c.row[tail & (ln == 0)]] = True
    heads_of = np.bincount(c.row[head], minlength=c.deg.size)
    if (none & (heads_of >= 3)).any():
        found.add("owner holds none of a row that runs through three later items")
    if (whole & (ln > 0) & (c.se + c.row == d1 - 1) & (d1 == (c.item + 1) * chunk)).any():
        found.add("row ending on an item's last token")
    items_head = set(c.item[head].tolist())
    items_tail = set(c.item[tail & (ln > 0)].tolist())
    if items_head & items_tail:
        found.add("item with a head and a tail")
    if items_head - set(c.owner.tolist()):
        found.add("item with a head and no owned row")
    tokens = np.bincount(c.item, weights=ln, minlength=c.n_items) \
        + np.bincount(c.owner, minlength=c.n_items)
    if ((tokens[c.owner] == 1) & (c.deg == 0)).any():
        found.add("item whose only token is an empty row's")
    pieces_of = np.bincount(c.row[ln > 0], minlength=c.deg.size)
    if ((c.deg >= 2) & (pieces_of == c.deg)).any():
        found.add("row in as many pieces as edges")
    return found


ALL_CLASSES = frozenset(
    [f"whole row of {k}" for k in (32, 33, 512, 513)]
    + [f"head piece of {k}: an item inside one row" for k in (512, 513)]
    + [f"tail piece of {k}" for k in (32, 33)]
    + ["owner holds none of a row that runs through three later items",
       "row ending on an item's last token", "item with a head and a tail",
       "item with a head and no owned row", "item whose only token is an empty row's",
       "row in as many pieces as edges"])
