"""The size-then-fill getters of oxmpl_amd.capi against a fake library: a call with null buffers and capacity 0 learns the
count, a second call fills arrays of that size.  No library is loaded and no GPU is needed.

The fake's oxhip_*_get_* functions write the count on the sizing call and 1, 2, 3, ... into every buffer on the filling call;
it records, per call, which buffers were null and the capacity it was given."""
import ctypes as C

import numpy as np
import pytest

from oxmpl_amd import capi

DIM, P = 3, 1
# name of the library function: (leading arguments after the handle, element width of each buffer, capacity for count n)
SIZED = {
    "oxhip_rrt_batch_get_tree": (1, (DIM, 1), lambda n: n),
    "oxhip_rrt_batch_get_goal_tree": (1, (DIM, 1), lambda n: n),
    "oxhip_rrt_batch_get_path": (1, (DIM,), lambda n: n),
    "oxhip_rrt_batch_get_costs": (1, (1,), lambda n: n),
    "oxhip_rrt_batch_get_paths": (1, (DIM,), lambda n: n),                   # (the leading argument is the offsets array)
    "oxhip_rrt_batch_get_simplified_paths": (1, (DIM, 1), lambda n: n),
    "oxhip_rrt_batch_path_valid_matrix": (2, (1,), lambda n: n * n),         # counts waypoints L, fills L * L verdicts
    "oxhip_rrt_batch_get_revalidate_map": (1, (1, 1), lambda n: n),
}


class FakeLib:
    def __init__(self, count, sizing_status=capi.OK):
        self.count, self.sizing_status, self.calls = count, sizing_status, []

    def oxhip_status_string(self, status):
        return b"status"

    def oxhip_last_error_string(self):
        return b"x"

    def oxhip_rrt_batch_get_simplify_results(self, h, raw, simplified, checks):
        return capi.OK

    def __getattr__(self, name):
        if name not in SIZED:
            raise AttributeError(name)
        n_lead, widths, capacity_of = SIZED[name]

        def fn(h, *a):
            lead, bufs, cap, count = a[:n_lead], a[n_lead:n_lead + len(widths)], a[-2], a[-1]._obj
            assert len(a) == n_lead + len(widths) + 2
            self.calls.append((name, [b is None for b in bufs], cap))
            if name.endswith("paths"):     # the batch getters fill the offsets [P + 1] on every call
                lead[0][0], lead[0][1] = 0, self.count
            if all(b is None for b in bufs):
                count.value = self.count
                return self.sizing_status
            assert not any(b is None for b in bufs) and cap == capacity_of(self.count)
            for b, w in zip(bufs, widths):
                for i in range(cap * w):
                    b[i] = i + 1
            count.value = self.count
            return capi.OK
        return fn


def batch():
    b = object.__new__(capi.RRTBatch)      # no handle: close() has nothing to destroy
    b._h, b.dim, b.n_problems, b.space = C.c_void_p(), DIM, P, capi.SPACE_REAL_VECTOR
    return b


def rows(n, width=DIM):
    return (np.arange(n * width, dtype=np.float64) + 1.0).reshape(n, width)


def same(got, want, dtype):
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == np.shape(want), (got.dtype, got.shape)
    assert got.tolist() == np.asarray(want).tolist()


def check_tree(out, n):
    states, parents = out
    same(states, rows(n), np.float64)
    same(parents, np.arange(n) + 1, np.int32)


def check_path(out, n):
    same(out, rows(n), np.float64)


def check_costs(out, n):
    same(out, np.arange(n) + 1.0, np.float64)


def check_paths(out, n):
    offsets, r = out
    same(offsets, [0, n], np.uint64)
    same(r, rows(n), np.float64)


def check_simplified(out, n):
    offsets, r, idx, raw, simp, checks = out
    same(offsets, [0, n], np.uint64)
    same(r, rows(n), np.float64)
    same(idx, np.arange(n) + 1, np.uint32)
    same(raw, np.zeros(P), np.float64)
    same(simp, np.zeros(P), np.float64)
    same(checks, np.zeros(P), np.uint64)


def check_matrix(out, n):
    same(out, np.ones((n, n), dtype=bool), np.bool_)


def check_map(out, n):
    new_index, edge_ok = out
    same(new_index, np.arange(n) + 1, np.int32)
    same(edge_ok, np.ones(n, dtype=bool), np.bool_)


# getter: (call, the library function behind it, check of the result, a second call when the count is 0?)
GETTERS = {
    "tree": (lambda b: b.tree(0), "oxhip_rrt_batch_get_tree", check_tree, True),
    "goal_tree": (lambda b: b.goal_tree(0), "oxhip_rrt_batch_get_goal_tree", check_tree, True),
    "path": (lambda b: b.path(0), "oxhip_rrt_batch_get_path", check_path, False),
    "costs": (lambda b: b.costs(0), "oxhip_rrt_batch_get_costs", check_costs, True),
    "paths": (lambda b: b.paths(), "oxhip_rrt_batch_get_paths", check_paths, True),
    "simplified_paths": (lambda b: b.simplified_paths(), "oxhip_rrt_batch_get_simplified_paths", check_simplified, True),
    "path_valid_matrix": (lambda b: b.path_valid_matrix(0, 2), "oxhip_rrt_batch_path_valid_matrix", check_matrix, True),
    "revalidate_map": (lambda b: b.revalidate_map(0), "oxhip_rrt_batch_get_revalidate_map", check_map, True),
}


@pytest.mark.parametrize("count", [0, 3])
@pytest.mark.parametrize("getter", list(GETTERS))
def test_getter_sizes_then_fills(monkeypatch, getter, count):
    call, fn, check, fills_empty = GETTERS[getter]
    fake = FakeLib(count)
    monkeypatch.setattr(capi, "_lib", fake)
    out = call(batch())
    check(out, count)
    n_bufs = len(SIZED[fn][1])
    assert fake.calls[0] == (fn, [True] * n_bufs, 0)                       # the sizing call: null buffers, capacity 0
    if count or fills_empty:
        assert fake.calls[1:] == [(fn, [False] * n_bufs, SIZED[fn][2](count))]
    else:
        assert fake.calls[1:] == []                                        # an empty path is not fetched


@pytest.mark.parametrize("getter", [g for g in GETTERS if g != "costs"])
def test_sizing_call_may_answer_capacity(monkeypatch, getter):
    """ERR_CAPACITY is the library's answer to a buffer that is too small, which a null buffer is.  (costs' sizing call is
    answered OK by the library and was checked for exactly that: not pinned either way.)"""
    call, fn, check, _ = GETTERS[getter]
    monkeypatch.setattr(capi, "_lib", FakeLib(3, sizing_status=capi.ERR_CAPACITY))
    check(call(batch()), 3)


@pytest.mark.parametrize("status", [capi.ERR_BAD_ARG, capi.ERR_NO_SOLUTION_FOUND, capi.ERR_HIP])
@pytest.mark.parametrize("getter", list(GETTERS))
def test_any_other_status_of_the_sizing_call_raises(monkeypatch, getter, status):
    call, fn, _, _ = GETTERS[getter]
    fake = FakeLib(3, sizing_status=status)
    monkeypatch.setattr(capi, "_lib", fake)
    with pytest.raises(capi.OxhipError) as e:
        call(batch())
    assert e.value.status == status and len(fake.calls) == 1
