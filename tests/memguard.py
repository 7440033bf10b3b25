"""Poisoned, guarded memory for the binding's launches (a plain helper, like tests/numerics.py).

Every launch of maxk_cuda_kernels runs on memory from torch.empty / torch.empty_like: the
workspace, the plan buffers, the outputs.  torch's caching allocator hands out fresh zeroed
pages or the finite floats of the previous test, and a store past a buffer lands in its slack,
so neither a read of an unwritten slot nor a store next to a buffer shows.  An Arena stands in
for the two functions while an op runs:

layout    one uint8 tensor; allocations bump-pointer at 4096-B aligned offsets, each with a guard
          band of its own before it ([off - 4096, off)) and after it (from payload byte n
          exactly, through the slack up to the next 4096 boundary, plus 4096 B).  4096 B is a
          choice, not a measurement: the widest row a kernel stores is D * 4 = 1024 B (a
          transport record 5k <= 1280 B), so a store misplaced by a row or a vector on either
          side lands inside.  Offsets stay 4096-aligned, so the library's 256-B and 16-B
          alignment requirements hold as they do with torch.empty.
canary    byte 0xFE in every byte of the arena that is not a payload: about -1.7e38 as an fp32
          word (a summed out-of-bounds read shows), negative as an int32, unlike every fill.
fills     zero   0x00: an unwritten index reads as 0, a valid row; an unwritten float is 0.
          ones   0xFF: an unwritten float is NaN; an unwritten int32 is -1 ("nothing to do"
                 for a fixup that skips row < 0, which is why zero is needed as well).
          stale  the payloads of the previous run of the same call sequence on another problem
                 of identical shapes -- the training loop: every index left over is valid for
                 these shapes, every float finite and wrong.
          An unwritten index is therefore 0, -1 (one element before the buffer: in the guard)
          or valid for the shapes.  No pattern whose int32 word is a large positive number
          (0x7F.., Inf, canonical NaN) belongs here: it could send a kernel far out of bounds.
          For the same reason a stale run whose allocation sizes differ from the run before
          raises at the allocation, before anything is launched on shifted leftovers.

run_regimes(op, inputs_factory) runs an op in all three and checks guards and inputs.
"""
from __future__ import annotations

import contextlib
import sys
from collections import namedtuple

import torch

GUARD = 4096
ALIGN = 4096
CANARY = 0xFE
FILL = {"zero": 0x00, "ones": 0xFF}
REGIMES = ("zero", "stale", "ones")

Alloc = namedtuple("Alloc", "ordinal offset nbytes site")


class ArenaExhausted(MemoryError):
    pass


class SequenceChanged(AssertionError):
    """A stale run asked for other sizes than the run whose payloads it is to inherit."""


class GuardDamaged(AssertionError):
    def __init__(self, alloc, side, offset, value):
        self.alloc, self.side, self.offset, self.value = alloc, side, offset, value
        if alloc is None:
            msg = f"arena byte {offset} outside every guard band changed to {value:#04x}"
        else:
            msg = (f"guard {side} allocation #{alloc.ordinal} ({alloc.nbytes} B, from "
                   f"{alloc.site}) damaged: first changed byte at payload offset {offset} "
                   f"(now {value:#04x})")
        super().__init__(msg)


class InputModified(AssertionError):
    pass


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


_ITEMSIZE: dict = {}


def _itemsize(dtype):
    if dtype not in _ITEMSIZE:
        _ITEMSIZE[dtype] = torch.zeros((), dtype=dtype).element_size()
    return _ITEMSIZE[dtype]


def _site():
    """file:line (function) of the nearest caller outside this module."""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == _site.__code__.co_filename:
        f = f.f_back
    if f is None:
        return "?"
    return f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"


def _shape(args):
    """The sizes of a plain torch.empty call (varargs or one tuple / list), else None."""
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if all(isinstance(a, int) and not isinstance(a, bool) for a in args):
        return tuple(int(a) for a in args)
    return None


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.buf = torch.full((_up(int(nbytes)),), CANARY, dtype=torch.uint8, device=self.device)
        self.allocs: list = []
        self.previous: list = []  # the sizes of the last finished run
        self.regime = None
        self.top = 0
        self.peak = 0             # largest extent any run reached, in bytes
        self._orig = None

    # ------------------------------------------------------------------------- the run
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def begin(self, regime):
        if regime not in REGIMES:
            raise ValueError(regime)
        if regime == "stale" and not self.previous:
            raise SequenceChanged("a stale run needs a finished run before it")
        self._sync()
        self.regime = regime
        self.allocs = []
        self.top = 0
        if regime != "stale":  # one fill: every byte outside the payloads to come is canary
            self.buf.fill_(CANARY)

    @contextlib.contextmanager
    def active(self, regime):
        """torch.empty / torch.empty_like served from the arena until the block ends."""
        self.begin(regime)
        self._orig = (torch.empty, torch.empty_like)
        torch.empty, torch.empty_like = self._empty, self._empty_like
        try:
            yield self
        finally:
            torch.empty, torch.empty_like = self._orig
            self._orig = None
            self.previous = [a.nbytes for a in self.allocs]

    def _take(self, nbytes, site):
        i = len(self.allocs)
        if self.regime == "stale" and (i >= len(self.previous) or self.previous[i] != nbytes):
            raise SequenceChanged(
                f"stale run: allocation #{i} asks {nbytes} B at {site}, the run before it "
                f"{self.previous[i] if i < len(self.previous) else 'nothing'}")
        off = self.top + GUARD
        end = _up(off + nbytes) + GUARD
        if end > self.buf.numel():
            raise ArenaExhausted(f"arena of {self.buf.numel()} B exhausted: allocation #{i} of "
                                 f"{nbytes} B at {site} would end at {end}")
        self.allocs.append(Alloc(i, off, nbytes, site))
        self.top = end
        self.peak = max(self.peak, end)
        if self.regime == "stale":  # the payload stays; both bands are rewritten
            self.buf[off - GUARD:off].fill_(CANARY)
            self.buf[off + nbytes:end].fill_(CANARY)
        elif nbytes:
            self.buf[off:off + nbytes].fill_(FILL[self.regime])
        return self.buf[off:off + nbytes]

    def _mine(self, device):
        if device is None:
            get = getattr(torch, "get_default_device", None)
            device = get() if get is not None else torch.device("cpu")
        device = torch.device(device)
        if device.type != self.device.type:
            return False
        if device.type == "cuda" and device.index is None:
            return self.device.index == torch.cuda.current_device()
        return device.index == self.device.index

    def _view(self, shape, dtype, site):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        n = 1
        for s in shape:
            n *= s
        return self._take(n * _itemsize(dtype), site).view(dtype).view(shape)

    def _empty(self, *args, **kw):
        shape = _shape(args)
        if shape is None or not set(kw) <= {"dtype", "device"} or not self._mine(kw.get("device")):
            return self._orig[0](*args, **kw)
        return self._view(shape, kw.get("dtype"), _site())

    def _empty_like(self, t, *args, **kw):
        if (args or not set(kw) <= {"dtype", "device"} or not isinstance(t, torch.Tensor)
                or not t.is_contiguous() or not self._mine(kw.get("device", t.device))):
            return self._orig[1](t, *args, **kw)
        return self._view(tuple(t.shape), kw.get("dtype", t.dtype), _site())

    # ------------------------------------------------------------------------- the check
    def check(self):
        """Every byte of the arena outside the payloads still holds the canary (one device-side
        comparison), else GuardDamaged naming the allocation, the side and the first byte."""
        self._sync()
        bad = self.buf != CANARY
        for a in self.allocs:
            if a.nbytes:
                bad[a.offset:a.offset + a.nbytes] = False
        if not bool(bad.any()):
            return
        i = int(bad.nonzero()[0])
        value = int(self.buf[i])
        for a in self.allocs:
            end = _up(a.offset + a.nbytes) + GUARD
            if a.offset - GUARD <= i < a.offset:
                raise GuardDamaged(a, "before", i - a.offset, value)
            if a.offset + a.nbytes <= i < end:
                raise GuardDamaged(a, "after", i - a.offset, value)
        raise GuardDamaged(None, None, i, value)

    def untouched(self, first=0):
        """After a zero or ones run: every payload byte of the allocations from ordinal `first`
        on still holds the fill (first = 0, with check(): nothing in the arena was written)."""
        self._sync()
        fill = FILL[self.regime]
        if first == 0:
            return not bool(((self.buf != CANARY) & (self.buf != fill)).any())
        return all(bool((self.buf[a.offset:a.offset + a.nbytes] == fill).all())
                   for a in self.allocs[first:])

    def owns(self, t):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            return False
        p, base = t.data_ptr(), self.buf.data_ptr()
        return base <= p < base + self.buf.numel()


# ------------------------------------------------------------------------------- run_regimes
def tensors(tree):
    """The tensors of a nested tuple / list / dict, in order."""
    if isinstance(tree, torch.Tensor):
        yield tree
    elif isinstance(tree, dict):
        for v in tree.values():
            yield from tensors(v)
    elif isinstance(tree, (tuple, list)):
        for v in tree:
            yield from tensors(v)


def copy_out(tree):
    """The same nest with every tensor cloned (out of the arena)."""
    if isinstance(tree, torch.Tensor):
        return tree.detach().clone()
    if isinstance(tree, dict):
        return {k: copy_out(v) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return type(tree)(copy_out(v) for v in tree)
    return tree


def raw(t):
    """A tensor's bytes (its elements in logical order) as a flat uint8 tensor: NaN == NaN."""
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1).to(torch.uint8)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


def run_once(arena, regime, op, inputs):
    """op(*inputs) under the arena in one regime: guards checked, inputs compared byte for byte
    with their snapshot; returns the outputs copied out of the arena."""
    ins = list(tensors(inputs))
    for t in ins:
        assert not arena.owns(t), "inputs are built outside the arena"
    snap = [raw(t).clone() for t in ins]
    with arena.active(regime):
        out = op(*inputs) if isinstance(inputs, (tuple, list)) else op(inputs)
    arena.check()
    for i, (t, s) in enumerate(zip(ins, snap)):
        if not torch.equal(raw(t), s):
            j = int((raw(t) != s).nonzero()[0])
            raise InputModified(f"input #{i} ({tuple(t.shape)} {t.dtype}) modified by the op "
                                f"(regime {regime}): first changed byte {j}")
    return copy_out(out)


def run_regimes(op, inputs_factory, arena, regimes=REGIMES):
    """{regime: outputs} of op in the regimes zero, stale, ones.

    inputs_factory(primer) builds fresh device inputs outside the arena on every call -- fresh
    graph tensors above all: the binding's caches are keyed on tensor identity, and a plan
    cached on an earlier run would be a view of arena memory refilled since.  primer=True asks
    for the other problem of identical shapes (another graph where the shapes allow it, other
    values and selectors otherwise) whose run, on zero-filled memory like a first training
    step's fresh pages, leaves the payloads the stale run starts from."""
    results = {}
    for regime in regimes:
        if regime == "stale":
            run_once(arena, "zero", op, inputs_factory(True))
        results[regime] = run_once(arena, regime, op, inputs_factory(False))
    return results
