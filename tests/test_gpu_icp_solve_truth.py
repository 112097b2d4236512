"""Both ICP solvers on the device - icp_step_row (16 lanes) and icp_step (one lane), through cd_icp_solve_batch - held to the
float64 Umeyama of tests/icp_solve_reference.py on the case set of tests/icp_solve_cases.py: one launch of 2 500 records per
parameter set, bounded and unbounded, over the five criteria sets.  The assertions are those of
tests/test_icp_solve_truth_cpu.py, which applies them to the same header on the host and to the CPU oracle and measures the
tolerances with the oracle: orthonormality, det R > 0 wherever S1 / S0 > 1e-4 (for rank <= 1 the sign is pcl::umeyama's own, from
the float32 determinant of a singular matrix, and is reported only), optimality, the rotation against R* within the perturbation
bound, the translation within its derived bound, and the convergence tail bit for bit."""
import pytest

import icp_solve_cases as CS
import icp_solve_reference as REF
from perception_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return REF.with_truth(CS.case_set())


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("crit", CS.CRITERIA, ids=[c[0] for c in CS.CRITERIA])
def test_row_and_lane_meet_the_truth(cases, crit, bounded):
    row, lane, done, _ = capi.icp_solve_batch(cases["sums"], cases["n"], cases["states"], bounded=bounded, **crit[1])
    c = REF.criteria(**crit[1])
    solved = ~((cases["n"] < 3) & bounded)
    for who, out, dn in (("row", row, done[:, 0]), ("lane", lane, done[:, 1])):
        REF.assert_solve(out["T"], cases, who, solved)
        bad, exits = REF.tail_mismatches(out, dn, cases["states"], cases["sums"], cases["n"], c, bounded)
        assert not bad, (who, len(bad), bad[:8], exits)
        assert exits["stop"] == (int((cases["n"] < 3).sum()) if bounded else 0) and exits["open"] > 0
