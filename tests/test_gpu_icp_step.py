"""Every exit of icp_step (icp_solve.hpp: one PCL iteration's state update) through every ICP driver.

The drivers share one implementation of the update; what differs is who calls it and where its `done` goes.  Each case below
makes ONE branch of DefaultConvergenceCriteria::hasConverged (or rule C8's stop) end a tiny ICP, and every driver must return the
oracle's record exactly.  The parameters were chosen with the oracle on the CPU: each run stops below its iteration limit, and
with the named criterion switched off the same source runs on (the counts are in CASES) - so the hard-coded iteration count
fails a case that stops by another branch.  Each case also runs with a bound that rejects nothing (10 m), which takes the
BOUNDED instantiation of the same kernels to the same record."""
import numpy as np
import pytest

from perception_amd import capi, templates
from test_gpu_icp_corr import GENERIC, LAT, cluster_near, fitness, make_ctx

gpu = pytest.mark.gpu   # (the first test only asks the oracle and runs everywhere)

# name -> (source, icp_max_iterations, icp_transformation_epsilon, icp_euclidean_fitness_epsilon, the oracle's iterations)
#   limit    : both epsilons tiny; without the limit of 2 the oracle runs 17 iterations
#   trans    : the rotation / translation test; with icp_transformation_epsilon = 0 the oracle runs 17 iterations
#   relative : |mse - prev| / prev < 0.1; with icp_euclidean_fitness_epsilon = 0 the oracle runs 17 iterations
#   absolute : an exact subset of the template, both epsilons 0: the relative test (x < 0) can never hold and the
#              transformation test only for an exact identity step, which test_cases_stop_by_the_branch_they_name rules out;
#              the MSE is 0 in iteration 1 and below 1e-12 in iteration 2
CASES = {"limit": ("near", 2, 1e-30, 1e-30, 2),
         "trans": ("near", 50, 1e-6, 0.0, 9),
         "relative": ("near", 50, 0.0, 0.1, 5),
         "absolute": ("subset", 50, 0.0, 0.0, 2)}
NPTS = 300


def params(mi, te, fe):
    p = capi.default_params()
    p.icp_max_iterations, p.icp_transformation_epsilon, p.icp_euclidean_fitness_epsilon = mi, te, fe
    return p


@pytest.fixture(scope="module")
def tpl():
    return templates.template_xyz32(**templates.DEFAULT_TEMPLATE)


@pytest.fixture(scope="module")
def sources(tpl):
    rng = np.random.default_rng(5)
    return {"near": cluster_near(tpl, NPTS, 1), "subset": tpl[rng.choice(len(tpl), NPTS, replace=False)].copy()}


@pytest.fixture(scope="module")
def expected(O, tpl, sources):
    """The oracle's record of every case, computed once."""
    out = {}
    for name, (src, mi, te, fe, _) in CASES.items():
        st, r, _ = O.icp(tpl, sources[src], params(mi, te, fe), nn_mode=1)
        assert st == 0
        out[name] = r
    return out


@pytest.fixture(scope="module")
def contexts(tpl):
    """One context per driver mode, made at first use (the mode is read from the environment when a context is created)."""
    made = {}

    def get(mode):
        if mode[0] not in made:
            with pytest.MonkeyPatch.context() as mp:
                made[mode[0]] = make_ctx(mp, mode[1], {0: tpl}, max_points=NPTS)
        return made[mode[0]]
    yield get
    for c in made.values():
        c.close()


def test_cases_stop_by_the_branch_they_name(O, tpl, sources, expected):
    for name, (src, mi, te, fe, iters) in CASES.items():
        assert (expected[name].iterations, expected[name].converged) == (iters, 1), name
        assert iters < mi or name == "limit"
    run = lambda src, mi, te, fe: O.icp(tpl, sources[src], params(mi, te, fe), nn_mode=1)[1]
    assert run("near", 50, 1e-30, 1e-30).iterations > CASES["limit"][4]
    assert run("near", 50, 0.0, 0.0).iterations > max(CASES["trans"][4], CASES["relative"][4])
    # absolute: the step that ended it was not an exact identity (which is all the transformation test accepts at epsilon 0)
    assert list(run("subset", 1, 0.0, 0.0).T) != list(expected["absolute"].T)


@gpu
@pytest.mark.parametrize("dist", [None, 10.0], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", [LAT] + GENERIC, ids=lambda m: m[0])
def test_every_convergence_branch_in_every_driver(contexts, sources, expected, mode, case, dist):
    src, mi, te, fe, iters = CASES[case]
    c, ro = contexts(mode), expected[case]
    c.set_icp_max_correspondence_distance(dist)
    st, r, _ = c.icp(0, sources[src], params(mi, te, fe))
    assert st == capi.CD_OK
    assert (r.iterations, r.converged) == (iters, 1)
    assert list(r.T) == list(ro.T) and (r.iterations, r.converged) == (ro.iterations, ro.converged)
    assert r.fitness == ro.fitness


@gpu
@pytest.mark.parametrize("mode", [LAT] + GENERIC, ids=lambda m: m[0])
def test_too_few_correspondences_stop_the_bounded_step(O, contexts, tpl, mode):
    """Rule C8 inside a BOUNDED run: 5 cm off the bottom face with a bound of 1 mm nothing is kept, and the step stops the ICP
    before the update - identity, no iteration, not converged; the fitness is still that of all points."""
    zb = tpl[:, 2].min()
    src = tpl[tpl[:, 2] == zb][::20] + np.float32([0.0, 0.0, 0.05])
    assert 3 <= len(src) <= NPTS
    c = contexts(mode)
    c.set_icp_max_correspondence_distance(1e-3)
    st, r, al = c.icp(0, src, capi.default_params(), want_aligned=True)
    assert st == capi.CD_ERR_FEW_CORRESPONDENCES
    assert (r.iterations, r.converged, r.accepted) == (0, 0, 0)
    assert list(r.T) == list(np.eye(4, dtype=np.float32).ravel())
    assert abs(r.fitness - fitness(O, tpl, src, np.eye(4))) <= 1e-12 * r.fitness
    assert np.array_equal(al, src)
