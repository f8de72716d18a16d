"""GPU: the kernels written once over SeqSpace<DIM> (oxmpl_amd/csrc/seq_space.hpp) give the same bits in every instantiation,
R^1..R^8 and SO(3): the single query (prm_query_kernel), the batch of one (prm_batch_flags_kernel) and the re-check
(prm_reval_valid_kernel, prm_reval_check_kernel / the SO(3) route through prm_so3_edge_kernel) against each other and against the
pure-Python restatement (tests/golden/make_golden.py, make_golden_so3.py).  The roadmaps are planted (set_roadmap), so nothing is
constructed: 1, 256 and 257 milestones are the i == 0 start-validity writer alone, the last lane of a block and the first lane
of a second block.  The scenes and their expectations: tests/prm_space_twins_helpers.py."""
import numpy as np
import pytest

from prm_revalidate_helpers import csr, edge_lists
from prm_space_twins_helpers import FRACTION, MAX_MILESTONES, SIZES, SPACES, assert_not_vacuous, expected, scene

pytestmark = pytest.mark.gpu

from oxmpl_amd import capi  # noqa: E402


def planted(sc):
    g = capi.PRMRoadmap(sc.dim, sc.bounds, sc.radius, MAX_MILESTONES, lvs_fraction=FRACTION,
                        space=capi.SPACE_SO3 if sc.space == 0 else capi.SPACE_REAL_VECTOR)
    g.set_spheres(sc.sphere_c, sc.sphere_r)
    if len(sc.box_lo):
        g.set_boxes(sc.box_lo, sc.box_hi)
    g.setup(sc.queries[0][0], sc.queries[0][1], sc.goal_radius)
    g.set_roadmap(sc.states, *csr(sc.lists))
    return g


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("space", SPACES)
def test_single_query_batch_and_recheck_agree_with_the_restatement(space, n):
    sc, want = scene(space, n), expected(space, n)
    assert_not_vacuous(space, n)
    g = planted(sc)
    for (start, goal), (start_valid, conn, goals) in zip(sc.queries, want["queries"]):
        g.set_problem(start, goal, sc.goal_radius)
        status, _ = g.solve()
        batch_status = g.solve_batch([start], [goal], [sc.goal_radius])[0]
        assert (status == capi.ERR_INVALID_START_STATE) == (batch_status == capi.ERR_INVALID_START_STATE) == (not start_valid)
        assert status == batch_status
        if not start_valid:
            conn, goals = [], []                         # an invalid start reports empty sets
        for got in (g.query_sets(), g.batch_query_sets(0)):
            assert got[0].tolist() == conn and got[1].tolist() == goals
    valid, kept_lists, _, _ = want["recheck"]
    mask, n_removed = g.revalidate()
    _, off, nb = g.roadmap()
    assert np.array_equal(mask, valid)
    assert edge_lists(off, nb) == kept_lists
    assert n_removed == sum(len(r) for r in sc.lists) - len(nb)
