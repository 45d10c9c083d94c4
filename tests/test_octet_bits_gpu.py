"""The eight-lane step kernels (csrc/octet.hpp) against golden BIT PATTERNS: every word of the state, of the per-step
records and of the flags after 40 env.step() calls, for small batches seeded so that each path of the substep is taken
-- calm balancing, a NEXT_STEP restart, both tires unloading, a not-admissible contact answered by an active set and one
that reaches the Gauss-Seidel sweeps, a hip or knee within reach of its stop -- at 8, 9 and 17 envs in the headline mode
(MODE_PENDULUM_AGENT), and for the fused rollout (4 steps per launch) and the Servos instantiation at 8 envs
(tests/octet_bits_cases.py). The fixture tests/golden/octet_bits.npz is recorded by tools/make_golden_octet_bits.py from
the library as it was BEFORE a change that must not move a bit (a shorter instruction stream, another block layout); the
rare-path census recorded with it proves that each case took its path, and must come out the same."""

import os

import numpy as np
import pytest

from tests import octet_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "octet_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {name: f[name] for name in f.files}


def test_fixture_covers_every_case(golden):
    names = {name.split("/")[0] for name in golden}
    assert names == {cases.case_id(case) for case in cases.CASES}


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_bits_match_the_recorded_library(case, golden):
    out = cases.run_case(case)
    problem = cases.path_taken(case, out)
    assert problem is None, problem
    for name, value in out.items():
        want = golden[f"{cases.case_id(case)}/{name}"]
        assert value.dtype == want.dtype and value.shape == want.shape, name
        differing = np.flatnonzero(value.ravel() != want.ravel())
        assert differing.size == 0, f"{name}: {differing.size} of {value.size} words differ, first at flat index {differing[0]}"
