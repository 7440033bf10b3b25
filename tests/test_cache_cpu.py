"""CPU: the tensor-keyed cache every plan, graph check and scaled-entry copy of the binding
lives in (maxk_cuda_kernels._cache.TensorCache), on CPU tensors with a counting build()."""
import gc

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)


@pytest.fixture
def cache():
    from maxk_cuda_kernels._cache import TensorCache
    return TensorCache()


class Build:
    """build() that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ["value", self.calls]


def test_binding_caches_are_this_type():
    import maxk_cuda_kernels as mk
    from maxk_cuda_kernels._cache import TensorCache
    for name in ("_CHECKED", "_PLAN_CACHE", "_DENSE_CACHE", "_BSORT_CACHE", "_PULL_CACHE",
                 "_HYBRID_CACHE", "_SCALED", "_LOCALITY"):
        assert isinstance(getattr(mk, name), TensorCache), name


def test_same_key_builds_once(cache):
    a, b, build = torch.zeros(3), torch.zeros(4), Build()
    v = cache.get((a, b), (8, 100), build)
    assert cache.get((a, b), (8, 100), build) is v
    assert build.calls == 1 and len(cache) == 1


def test_other_extra_is_another_entry(cache):
    a, b, build = torch.zeros(3), torch.zeros(4), Build()
    v = cache.get((a, b), (8,), build)
    w = cache.get((a, b), (16,), build)
    assert w is not v and build.calls == 2 and len(cache) == 2
    assert cache.get((a, b), (8,), build) is v and cache.get((a, b), (16,), build) is w
    assert build.calls == 2
    # the same tensors in another order are another key
    assert cache.get((b, a), (8,), build) is not v and len(cache) == 3


@pytest.mark.parametrize("which", [0, 1])
def test_in_place_write_rebuilds(cache, which):
    ts, build = (torch.zeros(3), torch.zeros(4)), Build()
    v = cache.get(ts, (1,), build)
    ts[which].add_(1)
    w = cache.get(ts, (1,), build)
    assert w is not v and build.calls == 2 and len(cache) == 1
    assert cache.get(ts, (1,), build) is w and build.calls == 2


def test_use_false_neither_reads_nor_stores(cache):
    a, build = torch.zeros(3), Build()
    assert cache.get((a,), (), build, use=False) == ["value", 1] and len(cache) == 0
    v = cache.get((a,), (), build)
    assert build.calls == 2 and len(cache) == 1
    assert cache.get((a,), (), build, use=False) is not v and build.calls == 3
    assert len(cache) == 1 and cache.get((a,), (), build) is v and build.calls == 3


def test_lookup_only_reads(cache):
    """lookup() is get()'s hit test alone: a caller may decide between it and the build."""
    a, build = torch.zeros(3), Build()
    assert cache.lookup((a,), (5,)) is None and len(cache) == 0
    v = cache.get((a,), (5,), build)
    assert cache.lookup((a,), (5,)) is v and cache.lookup((a,), (6,)) is None
    a.add_(1)
    assert cache.lookup((a,), (5,)) is None and build.calls == 1 and len(cache) == 1


@pytest.mark.parametrize("which", [0, 1, 2])
def test_entry_dies_with_any_key_tensor(cache, which):
    ts, build = [torch.zeros(3), torch.zeros(4), torch.zeros(5)], Build()
    cache.get(tuple(ts), (1,), build)
    cache.get(tuple(ts), (2,), build)
    other = torch.zeros(2)
    cache.get((other,), (), build)
    assert len(cache) == 3
    del ts[which]
    gc.collect()
    assert len(cache) == 1  # both entries of the dead tensor are gone, the other one stays
    assert cache.get((other,), (), build) == ["value", 3] and build.calls == 3


def test_inference_tensor_never_hits(cache):
    with torch.inference_mode():
        t = torch.zeros(3)
    assert t.is_inference()
    live, build = torch.zeros(3), Build()
    for n in (1, 2, 3):
        cache.get((live, t), (), build)
        assert build.calls == n and len(cache) == 0  # nothing is kept on an inference tensor
    del t
    gc.collect()
    assert len(cache) == 0


def test_recycled_id_is_not_the_dead_tensor(cache):
    """A new tensor at a dead key tensor's id() must not get that tensor's value: by the
    finalizer (the entry is gone once the tensor is), and by the weakref test where an entry
    is still there -- shown by filing a live tensor's entry under another tensor's key."""
    build = Build()
    a = torch.zeros(3)
    old_id, v = id(a), cache.get((a,), (7,), build)
    del a
    for _ in range(1000):  # CPython hands a freed block to the next object of that size
        b = torch.zeros(3)
        if id(b) == old_id:
            assert cache.get((b,), (7,), build) is not v
            break
        del b
    c, d = torch.zeros(3), torch.zeros(3)
    v = cache.get((c,), (7,), build)
    cache._entries[(id(d), 7)] = cache._entries[(id(c), 7)]  # what a recycled id would find
    calls = build.calls
    w = cache.get((d,), (7,), build)
    assert w is not v and build.calls == calls + 1
    assert cache.get((d,), (7,), build) is w and cache.get((c,), (7,), build) is v
