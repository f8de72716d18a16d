"""GPU: a PRM handle through its whole life -- construct_roadmap, set_roadmap, revalidate, grow_roadmap, prune, setup in the orders
no single call's tests reach ("Tests").  Every comparison is bit for bit.

test_filter_shape: prm_grow_filter_kernel at candidate counts on the wave and workgroup edges, with everything, nothing, one and
only new-new pairs surviving (tests/prm_lifecycle_shapes.py), against the host model's grow (tests/prm_lifecycle_model.py).
test_script: scripts that re-check, grow, prune and grow again across one and two moves of the capacity-sized buffers; after
every step the call's return values, get_roadmap and get_sizes against the model, and the TWIN CHECK: the veteran's get_roadmap is
planted into a fresh handle, and the two must agree on components, solve, solve_batch and solve_batch_shortest -- and, on copies
(a second handle that replays the script to this step), on a grow with a new stream and a re-check under scene B.  The twin's
services see only what get_roadmap shows, so any difference is state the veteran kept that it should not have: a stale binary32
shadow, weight array, label array, host copy or buffer pointer.
test_set_roadmap_after_growth: a handle grown past max_milestones cannot take its own roadmap back; a larger one can."""
import numpy as np
import pytest

import prm_lifecycle_shapes as ls
from helpers import bits
from prm_grow_helpers import check_rows
from prm_lifecycle_model import Refusal
from prm_revalidate_helpers import edge_lists
from prm_shortest_helpers import Batch, DISTANCE

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402

STATUS = {"BAD_ARG": capi.ERR_BAD_ARG, "CAPACITY": capi.ERR_CAPACITY, "UNSAMPLED_STATE_SPACE": capi.ERR_UNSAMPLED_STATE_SPACE}
SOLVE_STATUS = {"solved": capi.OK, "no_solution": capi.ERR_NO_SOLUTION_FOUND, "invalid_start": capi.ERR_INVALID_START_STATE}


def set_obstacles(h, sp, ob):
    h.set_spheres(np.array([c for c, _ in ob["spheres"]]).reshape(len(ob["spheres"]), sp["dim"]), [r for _, r in ob["spheres"]])
    if sp["kind"] != "so3" and ob["boxes"]:
        h.set_boxes(np.array([lo for lo, _ in ob["boxes"]]), np.array([hi for _, hi in ob["boxes"]]))


def setup_any(h):
    if h.space == capi.SPACE_SO3:
        h.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    else:
        h.setup([0.5] * h.dim, [9.5] * h.dim, 0.5)


def handle(sp, ob, max_milestones=None):
    """the model_of() of the device: the same space, seed, stream and obstacles, set up"""
    kw = dict(lvs_fraction=ls.FRACTION, seed=ls.SEED, stream=sp["stream"])
    if sp["kind"] == "so3":
        h = capi.PRMRoadmap(4, ls.SO3_UNBOUNDED, sp["radius"], max_milestones or sp["max_milestones"], space=capi.SPACE_SO3, **kw)
    else:
        h = capi.PRMRoadmap(sp["dim"], [(0.0, 10.0)] * sp["dim"], sp["radius"], max_milestones or sp["max_milestones"], knn_k=sp["knn_k"], **kw)
    set_obstacles(h, sp, ob)
    setup_any(h)
    return h


def assert_roadmap_equal(a, b):
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def grow_or_error(h, n_more, new_stream=None):
    try:
        return h.grow(n_more, new_stream=new_stream)
    except capi.OxhipError as e:
        return e


# ---------------------------------------------------------------------------------------------------------------- 1. the filter
@pytest.mark.parametrize("name", sorted(ls.SHAPES))
def test_filter_shape(name):
    sh, want = ls.shape(name), ls.grown(name)
    n_old = len(sh["states"])
    h = handle(sh["spec"], sh["obstacles"])
    h.set_roadmap(sh["states"], sh["offsets"], sh["nbrs"])
    assert h.grow(sh["n_more"], new_stream=sh["stream"]) == (want["added"], want["drawn"])
    rm = h.roadmap()
    assert_roadmap_equal(rm, want["roadmap"])
    assert h.sizes() == want["sizes"]
    rows = edge_lists(rm[1], rm[2])
    check_rows(rows)
    if "all_dropped" in name:                     # the old CSR comes back from the re-sort as it went in
        assert np.array_equal(rm[1][:n_old + 1], sh["offsets"]) and np.array_equal(rm[2], sh["nbrs"]) and h.sizes()[1] == len(sh["nbrs"])
    if name == "identity_257":                    # the filter ran and dropped nothing: the grow of a handle where it does not run
        twin = handle(sh["spec"], ls.NOTHING)
        twin.set_roadmap(sh["states"], sh["offsets"], sh["nbrs"])
        assert twin.grow(sh["n_more"], new_stream=sh["stream"]) == (want["added"], want["drawn"])
        assert_roadmap_equal(twin.roadmap(), rm)
        twin.close()
    valid, removed = h.revalidate()               # the rule a re-check keeps edges by: nothing goes
    assert removed == want["removed_after"] == 0 and np.array_equal(valid, want["valid_after"])
    assert_roadmap_equal(h.roadmap(), rm)
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the scripts
def apply(h, sp, t):
    """step t of a trace on the handle -> what the call returned, in the shape of the model's result"""
    op, a = t["op"], t["args"]
    if op == "construct":
        h.construct_roadmap()
    elif op == "setup":
        setup_any(h)
    elif op == "scene":
        set_obstacles(h, sp, t["obstacles"])
    elif op == "plant":
        h.set_roadmap(*a["roadmap"])
    elif op == "revalidate":
        return h.revalidate()
    elif op == "grow":
        return grow_or_error(h, a["n_more"], a.get("new_stream"))
    elif op == "prune":
        return h.prune(invalid=a.get("invalid", False), keep=a.get("keep"), min_size=a.get("min_size", 0), largest=a.get("largest", False))
    elif op == "components":
        return h.components()
    elif op == "fresh":
        f = handle(sp, t["obstacles"], max_milestones=a["n"])
        f.construct_roadmap()
        out = (f.roadmap(), f.sizes())
        f.close()
        return out
    return None


def assert_result(op, got, want):
    if isinstance(want, Refusal):
        assert isinstance(got, capi.OxhipError) and got.status == STATUS[want.status] and want.fragment in str(got)
    elif op == "grow":
        assert got == want
    elif op == "revalidate":
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    elif op == "prune":
        assert np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and (got[1], got[2]) == (want[1], want[2])
    elif op == "components":
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and tuple(got[2:]) == tuple(want[2:])
    elif op == "fresh":
        assert_roadmap_equal(got[0], want[0])
        assert got[1] == want[1]


def replay(name, upto):
    """a copy of the veteran: a second handle that runs the script's steps 0 .. upto"""
    sc, trace = ls.SCRIPTS[name], ls.run_script(name)
    h = handle(sc["spec"], ls.scene(sc["scene"], sc["start"]))
    for t in trace[:upto + 1]:
        if t["op"] != "fresh":
            apply(h, sc["spec"], t)
    return h


def components_equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def twin_check(name, veteran, k, t):
    """the veteran after step k against a fresh handle planted with its get_roadmap"""
    sc = ls.SCRIPTS[name]
    sp, ob = sc["spec"], t["obstacles"]
    rm, sizes = veteran.roadmap(), veteran.sizes()

    def planted():
        h = handle(sp, ob, max_milestones=max(sizes[0], sp["max_milestones"]))
        h.set_roadmap(*rm)
        return h
    twin = planted()
    assert components_equal(veteran.components(), twin.components())
    starts, goals, radii = ls.queries(sp, 8, 200 + k)
    for q in range(8):
        answers = []
        for h in (veteran, twin):
            h.set_problem(starts[q], goals[q], radii[q])
            answers.append(h.solve())
        assert answers[0][0] == answers[1][0] and np.array_equal(bits(answers[0][1]), bits(answers[1][1]))
        if t["marked"]:                           # and the golden generators' breadth-first search on the model's roadmap
            st, path = ls.model_solve(sp, ob, t["roadmap"], starts[q], goals[q], radii[q])
            assert answers[0][0] == SOLVE_STATUS[st] and np.array_equal(bits(answers[0][1]), bits(path))
    starts, goals, radii = ls.queries(sp, 32, 100 + k)
    for weights in (None, DISTANCE):
        V, T = Batch(veteran, starts, goals, radii, weights=weights), Batch(twin, starts, goals, radii, weights=weights)
        V.same_as(T)
        V.check_rows_are_milestones(rm[0])
        assert not t["marked"] or np.count_nonzero(V.status == capi.OK) >= 4     # (the CPU test asserts it of the model)
    assert components_equal(veteran.components(), twin.components())             # the kept labels, read a second time
    assert_roadmap_equal(veteran.roadmap(), rm)
    assert veteran.sizes() == sizes
    if t["marked"]:                               # the calls that change the roadmap, on copies: the veteran goes on from where it was
        copy = replay(name, k)
        assert_roadmap_equal(copy.roadmap(), rm)
        grown = [grow_or_error(h, 20, new_stream=11) for h in (copy, twin)]
        if isinstance(grown[0], capi.OxhipError):                                # (k-nearest over dead milestones)
            assert isinstance(grown[1], capi.OxhipError) and grown[0].status == grown[1].status
        else:
            assert grown[0] == grown[1] and grown[0][0] == 20
        assert_roadmap_equal(copy.roadmap(), twin.roadmap())
        assert copy.sizes()[:2] == twin.sizes()[:2]                              # (the twin's n_samples began at 0)
        for h in (copy, twin):
            set_obstacles(h, sp, ls.scene(sc["scene"], "B"))
        checked = [h.revalidate() for h in (copy, twin)]
        assert np.array_equal(checked[0][0], checked[1][0]) and checked[0][1] == checked[1][1]
        assert_roadmap_equal(copy.roadmap(), twin.roadmap())
        copy.close()
    twin.close()


@pytest.mark.parametrize("name", sorted(ls.SCRIPTS))
def test_script(name):
    sc, trace = ls.SCRIPTS[name], ls.run_script(name)
    sp = sc["spec"]
    h = handle(sp, ls.scene(sc["scene"], sc["start"]))
    for k, t in enumerate(trace):
        got = apply(h, sp, t)
        assert_result(t["op"], got, t["result"])
        if t["sizes"][0] == 0:                    # after setup(): nothing to read
            assert h.sizes() == (0, 0, 0)
            continue
        assert_roadmap_equal(h.roadmap(), t["roadmap"])      # (a refused step: the model's roadmap is the one before)
        assert h.sizes() == t["sizes"], (k, t["op"])
        if t["changed"]:
            twin_check(name, h, k, t)
    h.close()


# ---------------------------------------------------------------------------------------------------------------- 3. planting after growth
def test_set_roadmap_after_growth():
    sc = ls.SCRIPTS["setup_again"]
    sp, ob = sc["spec"], ls.scene(sc["scene"], "A")
    trace = ls.run_script("setup_again")
    h = handle(sp, ob)
    h.construct_roadmap()
    assert h.grow(800) == trace[1]["result"]
    rm, sizes = h.roadmap(), h.sizes()
    assert sizes[0] == 1100 > sp["max_milestones"]
    assert_roadmap_equal(rm, trace[1]["roadmap"])
    with pytest.raises(capi.OxhipError) as e:     # today's rule: set_roadmap is bounded by cfg.max_milestones, not by the capacity
        h.set_roadmap(*rm)
    assert e.value.status == capi.ERR_CAPACITY and "more milestones than max_milestones" in str(e.value)
    assert_roadmap_equal(h.roadmap(), rm)
    assert h.sizes() == sizes
    big = handle(sp, ob, max_milestones=1100)
    big.set_roadmap(*rm)
    assert_roadmap_equal(big.roadmap(), rm)
    assert big.sizes() == (sizes[0], sizes[1], 0)
    m = ls.model_of(sp, ob)                       # the refused call kept the stream's position: the next grow is the model's
    m.construct()
    m.grow(800)
    assert h.grow(7) == m.grow(7)
    assert_roadmap_equal(h.roadmap(), m.roadmap())
    assert h.sizes() == m.sizes()
    h.close(); big.close()
