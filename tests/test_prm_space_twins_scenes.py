"""CPU: the scenes of tests/test_gpu_prm_space_twins.py are not vacuous -- by the pure-Python restatement alone every case with a
full block of milestones has a start connection and a milestone that is none, a goal milestone and one that is none, an
invalid milestone, and a removed and a kept edge; the first query's start is valid, the second's is not."""
import pytest

from prm_space_twins_helpers import SIZES, SPACES, assert_not_vacuous


@pytest.mark.parametrize("space", SPACES)
def test_scene_is_not_vacuous(space):
    for n in SIZES:
        assert_not_vacuous(space, n)
