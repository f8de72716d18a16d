"""GPU: oxhip_prm_set_roadmap / oxhip_prm_revalidate (prm_revalidate.hip) on the shapes of
tests/prm_revalidate_limits_shapes.py, bit for bit and list for list against two references:
  (a) the CPU verdicts -- the C oracle over R^n, tests/golden/make_golden_so3.py over SO(3) -- through the plain filter
      (shapes.cpu_filter; tests/test_prm_revalidate_limits_model.py holds each shape to what it exists for), and
  (b) the plain filter over oxhip_rrt_batch_is_valid / oxhip_rrt_batch_check_motion of an RRT batch of the same space, bounds,
      fraction and obstacles, the motion taken from the higher index to the lower.
Every re-check asserts the valid mask and the invalid count, the removed entries, the edge lists, the states' bits, sizes(), and
that the rows are ascending and symmetric (`assert_recheck`).  No expectation comes from a device run of the code under test."""
import ctypes as C

import numpy as np
import pytest

import prm_revalidate_limits_shapes as shapes
from helpers import bits
from prm_revalidate_helpers import csr, edge_lists, plain_filter
from prm_revalidate_limits_shapes import cpu_filter

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- handles
def set_obstacles(h, S):
    """the scene's obstacles, replacing whatever the handle held (an empty table clears)"""
    h.set_spheres(S["sph_c"], S["sph_r"])
    if not S["so3"]:
        h.set_boxes(S["box_lo"], S["box_hi"])


def setup_any(g):
    if g.space == capi.SPACE_SO3:
        g.setup([0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], 0.2)
    else:
        g.setup([0.5] * g.dim, [9.5] * g.dim, 0.5)


def make_prm(S, cap=None, radius=None):
    cap = max(cap or len(S["states"]), 1)
    if S["so3"]:
        g = capi.PRMRoadmap(4, shapes.SO3_BOUNDS, radius or 0.5, cap, lvs_fraction=S["fraction"], space=capi.SPACE_SO3)
    else:
        g = capi.PRMRoadmap(S["dim"], S["bounds"], radius or 1.0, cap, lvs_fraction=S["fraction"])
    set_obstacles(g, S)
    setup_any(g)
    return g


def make_rrt(S):
    """an RRT batch of the shape's space, bounds, fraction and obstacles: the independent is_valid / check_motion"""
    if S["so3"]:
        b = capi.RRTBatch(4, shapes.SO3_BOUNDS, 0.5, 0.05, 1, max_nodes=64, lvs_fraction=S["fraction"], space=capi.SPACE_SO3)
    else:
        b = capi.RRTBatch(S["dim"], S["bounds"], 1.0, 0.05, 1, max_nodes=64, lvs_fraction=S["fraction"])
    if len(S["sph_r"]):
        b.set_spheres(S["sph_c"], S["sph_r"])
    if len(S["box_lo"]):
        b.set_boxes(S["box_lo"], S["box_hi"])
    return b


def independent_filter(rrt, states, lists):
    """(valid, filtered lists) from the RRT batch's own is_valid / check_motion, from = the higher index"""
    valid = rrt.is_valid(states)
    pairs = [(j, i) for j, row in enumerate(lists) for i in row if i < j and valid[i] and valid[j]]
    ok = {}
    if pairs:
        idx = np.array(pairs)
        ok = dict(zip(pairs, rrt.check_motion(states[idx[:, 0]], states[idx[:, 1]])))
    return valid, plain_filter(lists, valid, ok)


def plant(g, states, lists):
    off, nb = csr(lists)
    g.set_roadmap(states, off, nb)
    s, o, n = g.roadmap()
    assert np.array_equal(bits(s), bits(states)) and np.array_equal(o, off) and np.array_equal(n, nb)
    assert g.sizes() == (len(states), len(nb), 0)


def recheck(g):
    """oxhip_prm_revalidate with all three results: (valid mask, invalid milestones, removed entries)"""
    n = g.sizes()[0]
    valid = np.zeros(max(n, 1), dtype=np.uint8)
    n_invalid, removed = C.c_uint32(0xFFFFFFFF), C.c_uint64(0xFFFFFFFF)
    capi._check(capi.lib().oxhip_prm_revalidate(g._h, capi._p(valid, capi._u8p), C.byref(n_invalid), C.byref(removed)))
    assert set(np.unique(valid[:n])) <= {0, 1}
    return valid[:n].astype(bool), n_invalid.value, removed.value


def assert_recheck(g, S, states, lists, ref):
    """re-checks g, which holds (states, lists), in the scene S; `ref`: reference (a), shapes.cpu_filter of the same.  Returns the
    edge lists that are left"""
    rrt = make_rrt(S)
    valid_b, kept_b = independent_filter(rrt, states, lists)                               # reference (b)
    rrt.close()
    valid, n_invalid, removed = recheck(g)
    s2, off, nb = g.roadmap()
    got = edge_lists(off, nb)
    assert np.array_equal(valid, ref["valid"]) and np.array_equal(valid, valid_b), S["name"]
    assert n_invalid == np.count_nonzero(~ref["valid"]), S["name"]
    assert got == ref["kept"], S["name"]
    assert got == kept_b, S["name"]
    assert removed == sum(len(r) for r in lists) - len(nb), S["name"]
    assert np.array_equal(bits(s2), bits(states)), S["name"]                               # indices are stable, states untouched
    assert g.sizes() == (len(states), len(nb), 0) and int(off[0]) == 0 and int(off[-1]) == len(nb), S["name"]
    for u, row in enumerate(got):
        assert all(a < b for a, b in zip(row, row[1:])) and all(u in got[v] for v in row), (S["name"], u)
    return got


def plant_and_recheck(S, g=None):
    own = g is None
    g = make_prm(S) if own else g
    plant(g, S["states"], S["lists"])
    got = assert_recheck(g, S, S["states"], S["lists"], cpu_filter(S))
    if own:
        g.close()
    return got


# ---------------------------------------------------------------------------------------------------------------- A .. D
@pytest.mark.parametrize("dim,leg", shapes.A_LEGS, ids=["%s_%s" % ("so3" if d == 0 else "r%d" % d, leg) for d, leg in shapes.A_LEGS])
def test_every_space_and_obstacle_kind(dim, leg):
    plant_and_recheck(shapes.space_scene(dim, leg))


@pytest.mark.parametrize("n_spheres,with_boxes", shapes.B_LEGS)
def test_decisive_sphere_at_the_end_of_a_window(n_spheres, with_boxes):
    got = plant_and_recheck(shapes.window_scene(n_spheres, with_boxes))
    assert got[0] == [] and got[2] == [3]


def test_step_counts_either_side_of_an_integer():
    S = shapes.steps_scene()
    got = plant_and_recheck(S)
    for name, (j, i, _, _) in S["pairs"].items():
        assert (i in got[j]) == cpu_filter(S)["ok"][(j, i)], name


@pytest.mark.parametrize("dim", shapes.D_DIMS)
def test_milestones_outside_the_bounds(dim):
    plant_and_recheck(shapes.outside_scene(dim))


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("so3", [False, True], ids=["r3", "so3"])
@pytest.mark.parametrize("kind", shapes.E_KINDS)
def test_csr_shapes(kind, so3):
    base = shapes.csr_base(kind, so3)
    g = make_prm(base)
    for placement in shapes.E_PLACEMENTS:                # one handle: each placement plants the shape anew
        S = shapes.csr_scene(kind, so3, placement)
        set_obstacles(g, S)
        got = plant_and_recheck(S, g)
        if placement == "none":
            assert got == S["lists"]
        if placement == "all":
            assert not any(got)
    g.close()


# ---------------------------------------------------------------------------------------------------------------- F
def roadmap_of(g):
    s, off, nb = g.roadmap()
    return bits(s).copy(), off.copy(), nb.copy()


def assert_equals_fresh_handle(g, S, valid):
    """g, re-checked in S, holds what a fresh handle planted with S's roadmap and re-checked in S holds"""
    fresh = make_prm(S)
    plant(fresh, S["states"], S["lists"])
    v2, _, _ = recheck(fresh)
    assert np.array_equal(valid, v2) and g.sizes() == fresh.sizes()
    for a, b in zip(roadmap_of(g), roadmap_of(fresh)):
        assert np.array_equal(a, b)
    fresh.close()


@pytest.mark.parametrize("so3", [False, True], ids=["r3", "so3"])
def test_repeats_and_reuse_on_one_handle(so3):
    n0 = shapes.F_SIZES[0]
    S0, S1, S2 = (shapes.reuse_scene(so3, n0, level) for level in (0, 1, 2))
    st = S1["states"]
    g = make_prm(S1, cap=max(shapes.F_SIZES))
    plant(g, st, S1["lists"])
    kept1 = assert_recheck(g, S1, st, S1["lists"], cpu_filter(S1))
    before = roadmap_of(g)
    again = assert_recheck(g, S1, st, kept1, cpu_filter(S1, lists=kept1, key="again"))     # twice in one scene: nothing more goes
    assert again == kept1 and all(np.array_equal(a, b) for a, b in zip(before, roadmap_of(g)))
    set_obstacles(g, S2)                                                                   # S2 holds S1's obstacles and more
    kept2 = assert_recheck(g, S2, st, kept1, cpu_filter(S2, lists=kept1, key="after_s1"))
    assert kept2 == cpu_filter(S2)["kept"]                                                 # the plain filter of the ORIGINAL roadmap in S2
    set_obstacles(g, S0)                                                                   # no obstacle: nothing returns
    ref0 = cpu_filter(S0, lists=kept2, key="cleared")
    assert ref0["valid"].all()
    assert assert_recheck(g, S0, st, kept2, ref0) == kept2
    valid = None
    for n in shapes.F_SIZES:                                                               # 1,200, then 40, then 1,300 on the same handle
        S = shapes.reuse_scene(so3, n, 2)
        set_obstacles(g, S)
        plant(g, S["states"], S["lists"])
        assert_recheck(g, S, S["states"], S["lists"], cpu_filter(S))
        valid, _, removed = recheck(g)                                                     # (and once more: the mask again, nothing removed)
        assert removed == 0 and np.array_equal(valid, cpu_filter(S)["valid"])
        assert_equals_fresh_handle(g, S, valid)
    g.close()


# ---------------------------------------------------------------------------------------------------------------- G
def answers(g, queries):
    """what solve_batch and solve_batch_shortest return for the queries, as comparable arrays"""
    s, t, r = queries
    out = []
    for shortest in (False, True):
        st = (g.solve_batch_shortest if shortest else g.solve_batch)(s, t, r).copy()
        res = g.batch_results()
        off, nodes, rows = g.batch_paths()
        out += [st, res["path_len"], res["goal_node"], res["n_start"], res["n_goal"], off, nodes, bits(rows)]
        if shortest:
            out.append(bits(g.batch_costs()))
    return out


def test_refusals_across_blocks_leave_the_handle_alone():
    base = shapes.refusal_base()
    st, n = base["states"], shapes.G_N
    g = make_prm(base, cap=n, radius=1.5)                # n == max_milestones exactly
    plant(g, st, base["lists"])
    rng = np.random.default_rng(11)
    q = (rng.uniform(1.0, 9.0, size=(16, 3)), rng.uniform(1.0, 9.0, size=(16, 3)), np.full(16, 1.5))
    before, ans = roadmap_of(g), answers(g, q)           # (the last batch is the shortest-path one)
    assert np.count_nonzero(ans[0] == capi.OK) >= 4

    def untouched():
        assert all(np.array_equal(a, b) for a, b in zip(before, roadmap_of(g)))
        res = g.batch_results()
        assert np.array_equal(res["status"], ans[8]) and np.array_equal(bits(g.batch_costs()), ans[16])

    for name in shapes.REFUSALS:
        off, nb, (rule, row) = shapes.refusal(name)
        with pytest.raises(capi.OxhipError) as e:
            g.set_roadmap(st, off, nb)
        msg = str(e.value)
        assert e.value.status == capi.ERR_BAD_ARG and ("rule " + rule + " ") in msg and msg.endswith("row %d" % row), (name, rule, row, msg)
        untouched()
    with pytest.raises(capi.OxhipError) as e:            # one milestone more than max_milestones
        g.set_roadmap(np.vstack([st, st[:1]]), *csr(base["lists"] + [[]]))
    assert e.value.status == capi.ERR_CAPACITY
    untouched()
    a2 = answers(g, q)
    assert len(a2) == len(ans) and all(np.array_equal(x, y) for x, y in zip(a2, ans))
    # the full-size roadmap re-checked where it stands: four entries a row, 16 blocks of entries
    S = shapes.with_obstacles(base, "G_base_scene", ([st[256].copy(), shapes.on_edge(base, 1023, 0), shapes.on_edge(base, 256, 255)],
                                                     [0.3, shapes.THIN, shapes.THIN]))
    set_obstacles(g, S)
    got = assert_recheck(g, S, st, base["lists"], cpu_filter(S))
    assert got[256] == [] and 0 not in got[1023] and 255 not in got[256]
    g.close()


def test_accepted_edge_cases():
    cases = shapes.accepted_edge_cases()
    E = cases["empty_first_and_last_rows"]
    S = shapes.with_obstacles(E, "G_empty_ends_scene", ([E["states"][5].copy(), shapes.on_edge(E, 2, 1), shapes.on_edge(E, 1022, 1)],
                                                        [0.2, shapes.THIN, shapes.THIN]))
    got = plant_and_recheck(S)
    assert got[0] == got[-1] == got[5] == [] and 1 not in got[2] and 1 not in got[1022]
    Z = cases["no_entries"]                              # neighbours = NULL with zero entries: emit, scan and compaction are skipped
    g = make_prm(Z)
    g.set_roadmap(Z["states"], np.zeros(301, dtype=np.uint64), [])
    assert g.sizes() == (300, 0, 0)
    got = assert_recheck(g, Z, Z["states"], Z["lists"], cpu_filter(Z))
    assert not any(got)
    valid, n_invalid, removed = recheck(g)
    assert n_invalid == np.count_nonzero(~valid) >= 1 and removed == 0
    g.close()
