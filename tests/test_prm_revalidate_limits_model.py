"""CPU: every shape of tests/prm_revalidate_limits_shapes.py has the property it exists for, by the references alone -- the C oracle
(oracle_py.OracleRRT.is_valid / check_motion) over R^n, tests/golden/make_golden_so3.py (Cones, check_motion) over SO(3), and
prm_revalidate_helpers.plain_filter.  No GPU.  Each test prints its shape's counts (run with -s): invalid milestones, edges cut
between valid ends, edges kept; the run's output is the record.  tests/test_gpu_prm_revalidate_limits.py compares the device with
these verdicts.

What the shapes cannot show is said where it is computed: an odd entry count (a symmetric CSR without self-loops holds an even
number of entries, so 254 / 256 / 258 / 512 / 514 stand for "256, 257, 512"), and a sphere that the re-check's wider filter margin
(SeqSpace::motion_margin) decides: test_outside_bounds derives why no motion between two valid ends has one."""
import numpy as np
import pytest

import prm_revalidate_limits_shapes as shapes
from prm_revalidate_helpers import csr
from prm_revalidate_limits_shapes import cpu_filter


def entries(S):
    return sum(len(r) for r in S["lists"])


def assert_symmetric_ascending(lists):
    for u, row in enumerate(lists):
        assert row == sorted(set(row)) and u not in row
        assert all(u in lists[v] for v in row)


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("dim,leg", shapes.A_LEGS, ids=["%s_%s" % ("so3" if d == 0 else "r%d" % d, leg) for d, leg in shapes.A_LEGS])
def test_every_space_loses_a_milestone_and_an_edge_and_keeps_one(dim, leg):
    S = shapes.space_scene(dim, leg)
    f = cpu_filter(S)
    print(shapes.counts(S))
    assert_symmetric_ascending(S["lists"])
    assert len(S["lists"]) == shapes.A_N > 256 and entries(S) > shapes.A_N + 1
    assert (len(S["sph_r"]) > 0) == (leg != "boxes") and (len(S["box_lo"]) > 0) == (leg in ("boxes", "both"))
    assert f["invalid"] > 0 and f["cut"] > 0 and f["kept_edges"] > 0
    if leg == "both":
        fs, fb = cpu_filter(S, boxes=False), cpu_filter(S, spheres=False)
        by_sphere = [e for e, ok in f["ok"].items() if not ok and not fs["ok"][e] and fb["ok"][e]]
        by_box = [e for e, ok in f["ok"].items() if not ok and fs["ok"][e] and not fb["ok"][e]]
        print("   cut by a sphere alone %d, by a box alone %d" % (len(by_sphere), len(by_box)))
        assert by_sphere and by_box
        assert np.count_nonzero(~fs["valid"]) > 0 and np.count_nonzero(~fb["valid"]) > 0   # a milestone in a sphere, another in a box


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("n_spheres,with_boxes", shapes.B_LEGS)
def test_the_last_sphere_of_the_table_decides(n_spheres, with_boxes):
    S = shapes.window_scene(n_spheres, with_boxes)
    f = cpu_filter(S)
    print(shapes.counts(S))
    assert len(S["sph_r"]) == n_spheres and n_spheres - 1 in (62, 63, 64, 127, 128)
    assert f["valid"].all()
    assert f["ok"] == {(1, 0): False, (3, 2): True, (5, 4): not with_boxes, (7, 6): True}
    without_last = cpu_filter(S, n_spheres=n_spheres - 1)
    assert without_last["ok"][(1, 0)] and without_last["valid"].all()
    if with_boxes:
        assert len(S["box_lo"]) == 2 and n_spheres > 64 and cpu_filter(S, boxes=False)["ok"][(5, 4)]


# ---------------------------------------------------------------------------------------------------------------- C
def test_step_counts_either_side_of_an_integer():
    S = shapes.steps_scene()
    f = cpu_filter(S)
    print(shapes.counts(S))
    res, st = shapes.resolution(S), S["states"]
    assert f["valid"].all()
    for name, (j, i, n_steps, kept) in S["pairs"].items():
        got = shapes.steps(S, st[j], st[i])
        print("   %-10s dist / res = %.17g  steps %d  kept %s" % (name, shapes.distance(S, st[j], st[i]) / res, got, f["ok"][(j, i)]))
        assert got == n_steps and f["ok"][(j, i)] == kept, name
    j, i = S["pairs"]["duplicate"][:2]
    assert j > i and np.array_equal(st[j], st[i])
    for k in (1, 2):
        j, i = S["pairs"]["k%d_exact" % k][:2]
        assert shapes.distance(S, st[j], st[i]) / res == float(k)
    # the spheres decide by the extra state alone: without them every planted edge is kept
    assert all(cpu_filter(S, spheres=False)["ok"].values())


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("dim", shapes.D_DIMS)
def test_outside_bounds_both_verdicts_and_the_filter_margin(dim):
    S = shapes.outside_scene(dim)
    f = cpu_filter(S)
    print(shapes.counts(S))
    st = S["states"]
    assert {-50.0, 1e3, 1e5} <= set(st.reshape(-1)) and S["bounds"] == [(0.0, 10.0)] * dim
    assert f["valid"].all()
    want = dict(through=False, graze=False, miss=True, far=True)
    for name, (j, i, kind) in S["roles"].items():
        outside = lambda s: bool(((s < 0.0) | (s > 10.0)).any())   # noqa: E731
        assert outside(st[j]) and outside(st[i]) == name.startswith("out_out")
        n = shapes.steps(S, st[j], st[i])
        assert 2 <= n <= 200000
        assert f["ok"][(j, i)] == want[kind], name
        line = "   %-16s %-7s steps %6d kept %s" % (name, kind, n, f["ok"][(j, i)])
        if kind in ("graze", "miss"):
            # The filter keeps a sphere while d(centre, mid) <= r + dist / 2 + margin.  A sphere that hits a tested state s has
            # d(centre, mid) <= r + d(s, mid), and between valid ends s is not an end, so d(s, mid) <= dist / 2 - dist / steps: the
            # slack is at least dist / steps (about the resolution) however the sphere is placed, while the margin is 5e-7 dist + 1e-9
            # of the largest coordinate -- below a tenth of the resolution for every motion of at most 2e5 steps.  So no shape within
            # the step limit brings a decisive sphere within twice the margin of being dropped; this one comes as near as a sphere can.
            slack, margin = shapes.filter_slack(S, j, i, S["sphere_of"][name])
            step = shapes.distance(S, st[j], st[i]) / n
            line += "  filter slack %.6g = %.3f steps, margin %.6g: the shape does not reach twice the margin" % (slack, slack / step, margin)
            assert slack > 0.0 and margin > 0.0
            assert slack > 2.0 * margin           # stated plainly: not within twice the margin (see above)
            if name.startswith("out_in"):
                assert slack < 1.6 * step         # and no farther from it than the geometry forces
        print(line)
    assert set(f["ok"].values()) == {True, False}


# ---------------------------------------------------------------------------------------------------------------- E
def _empty_runs(lists):
    runs, run = [], 0
    for row in lists + [[0]]:
        if row:
            runs.append(run)
            run = 0
        else:
            run += 1
    return runs


def test_csr_shapes_have_their_structure():
    for kind in shapes.E_KINDS:
        lists = shapes.csr_lists(kind)
        assert_symmetric_ascending(lists)
        n, e = len(lists), sum(len(r) for r in lists)
        print("%-12s n %4d entries %4d" % (kind, n, e))
        assert e % 2 == 0                                       # why no shape has 257 entries
        if kind.startswith("entries_"):
            assert e == int(kind.split("_")[1])
    assert _empty_runs(shapes.csr_lists("front_empty"))[0] == 300 and len(shapes.csr_lists("front_empty")) == 365
    assert sorted(set(_empty_runs(shapes.csr_lists("inner_runs")))) == [0, 2, 70] and not _empty_runs(shapes.csr_lists("inner_runs"))[0]
    tail = shapes.csr_lists("tail_empty")
    assert all(not r for r in tail[65:]) and len(tail) + 1 > sum(len(r) for r in tail) + 256 * 2   # two whole blocks of offsets only
    assert all(len(r) == 23 for r in shapes.csr_lists("k24"))
    assert len(shapes.csr_lists("hub_first")[0]) == 300 == len(shapes.csr_lists("hub_last")[300])


@pytest.mark.parametrize("so3", [False, True], ids=["r3", "so3"])
@pytest.mark.parametrize("kind", shapes.E_KINDS)
def test_csr_shapes_are_cut_where_they_are_meant_to_be(kind, so3):
    lists = shapes.csr_lists(kind)
    n_entries, n_edges = sum(len(r) for r in lists), sum(len(r) for r in lists) // 2
    first, last, pred = (shapes.entry_edge(lists, e) for e in (0, n_entries - 1, n_entries - 2))
    assert last != pred
    for placement in shapes.E_PLACEMENTS:
        S = shapes.csr_scene(kind, so3, placement)
        f = cpu_filter(S)
        print(shapes.counts(S))
        assert f["valid"].all() and len(S["sph_r"]) > 0 and len(f["ok"]) == n_edges     # every milestone stays valid
        cut = sorted(e for e, ok in f["ok"].items() if not ok)
        assert cut == dict(first=[first], last=[last], pred=[pred], all=sorted(f["ok"]), none=[])[placement]
        if placement == "pred":
            assert f["ok"][last]
        if placement == "all":
            assert f["kept_edges"] == 0 and len(S["sph_r"]) == n_edges


# ---------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("so3", [False, True], ids=["r3", "so3"])
@pytest.mark.parametrize("n", shapes.F_SIZES)
def test_reuse_scenes_are_nested_and_not_vacuous(n, so3):
    S0, S1, S2 = (shapes.reuse_scene(so3, n, level) for level in (0, 1, 2))
    f0, f1, f2 = cpu_filter(S0), cpu_filter(S1), cpu_filter(S2)
    for S in (S0, S1, S2):
        print(shapes.counts(S))
    assert len(S0["sph_r"]) == 0 and f0["valid"].all() and f0["kept"] == S0["lists"]
    assert np.array_equal(S2["sph_c"][:len(S1["sph_c"])], S1["sph_c"]) and len(S2["sph_r"]) > len(S1["sph_r"])     # S2 holds S1
    for f in (f1, f2):
        assert f["invalid"] > 0 and f["cut"] > 0 and f["kept_edges"] > 0
    assert f2["invalid"] > f1["invalid"] and f2["kept_edges"] < f1["kept_edges"]
    assert all(set(a) <= set(b) for a, b in zip(f2["kept"], f1["kept"]))
    # re-checking in S1, then in S2, is the plain filter of the original roadmap in S2
    assert cpu_filter(S2, lists=f1["kept"], key="after_s1")["kept"] == f2["kept"]
    # and a second re-check in the same scene removes nothing
    assert cpu_filter(S1, lists=f1["kept"], key="again")["kept"] == f1["kept"]


# ---------------------------------------------------------------------------------------------------------------- G
def test_refusal_shapes_break_what_they_name():
    base, n = shapes.refusal_base(), shapes.G_N
    off, nb = csr(base["lists"])
    assert shapes.first_violation(n, off, nb) is None
    assert n >= 1000 and len(nb) == 4096 >= 3 * 256
    assert shapes.row_entry_block(base["lists"], 255) == 3 and shapes.row_entry_block(base["lists"], 256) == 4
    for S in shapes.accepted_edge_cases().values():
        assert shapes.first_violation(len(S["lists"]), *csr(S["lists"])) is None
    edge = shapes.accepted_edge_cases()["empty_first_and_last_rows"]["lists"]
    assert not edge[0] and not edge[-1] and all(edge[1:-1])
    last = n - 1
    for name in shapes.REFUSALS:
        o, b, want = shapes.refusal(name)
        print("%-40s -> %s, row %d" % (name, *want))
        assert int(o[-1]) == len(b)                             # the call reads offsets[n] neighbours
        rule = next((r for r in shapes.RULES[1:] if name.startswith(r)), None)
        if name == "offsets_order_0_last":
            assert want == ("offsets_start", 0)                 # offsets[0] > offsets[1] needs offsets[0] != 0
        elif rule and name.endswith("_255_256"):
            assert want == (rule, 255)
        elif rule and name.endswith("_0_last"):
            assert want == (rule, 0)
        elif rule and name.endswith("_256_last"):
            assert want == (rule, 256)
        elif rule and name.endswith("_last"):
            assert want == (rule, last)
    assert shapes.refusal("offsets_start")[2] == ("offsets_start", 0)
    assert shapes.refusal("offsets_start_and_order")[2] == ("offsets_start", 0)
    assert shapes.refusal("all_entry_rules")[2] == ("neighbour_range", 900)          # though the other rules break in lower rows
    assert shapes.refusal("unsorted_then_lower_rows_asymmetric")[2] == ("unsorted", 800)
    assert shapes.refusal("self_loop_then_lower_rows_unsorted")[2] == ("self_loop", 1000)
    assert shapes.refusal("unsorted_row_hides_asymmetry")[2] == ("unsorted", 513)
    # the offending entry is the very last of the roadmap
    assert int(shapes.refusal("neighbour_range_last")[1][-1]) == n
    u = shapes.refusal("unsorted_last")[1]
    assert u[-1] < u[-2]
    o = shapes.refusal("offsets_order_last")[0]
    assert o[last] > o[n] and all(o[i] <= o[i + 1] for i in range(last))


def test_rule_checker_on_small_cases():
    fv = shapes.first_violation
    assert fv(3, [0, 1, 2, 2], [1, 0]) is None
    assert fv(3, [1, 1, 2, 2], [1, 0]) == ("offsets_start", 0)
    assert fv(3, [0, 2, 1, 2], [1, 0]) == ("offsets_order", 1)
    assert fv(3, [0, 1, 2, 2], [3, 0]) == ("neighbour_range", 0)
    assert fv(3, [0, 1, 2, 2], [0, 0]) == ("self_loop", 0)
    assert fv(3, [0, 2, 3, 4], [2, 1, 0, 0]) == ("unsorted", 0)
    assert fv(3, [0, 1, 1, 1], [1]) == ("asymmetric", 0)
    assert fv(3, [0, 2, 3, 4], [1, 1, 0, 0]) == ("unsorted", 0)      # a repeated neighbour is not strictly ascending
