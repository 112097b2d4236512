"""A single-face cluster end to end through every ICP driver.  The default template is a lattice with one face per axis; a cluster
that sees one face pairs with template points that are exactly coplanar, sigma = cov(q, p) has rank 2 and the rotation comes from
the rank == 2 / det U det V branch of the solve - the branch production takes.  Source: the interior points of one face (300 of
the large one, all of the two thin ones), moved by up to 0.1 degrees and 0.3 mm, three seeds each (icp_solve_cases.planar_scenes).
Input assertion, float64 brute force: every moved point's nearest template point is the point it came from, so the first
iteration's pairs are known.  With icp_max_iterations = 1 the record's final transformation must agree with the float64 Umeyama of
(moved, original) within the rotation bound of tests/icp_solve_reference.py and the translation bound plus |dR| |mp| - hence with
the inverse motion - and det R > 0; with the default limit the ICP converges and T and the pose agree with the inverse motion
and the motion to POSE_TOL.  tests/test_icp_solve_truth_cpu.py holds the CPU oracle to the same."""
import pytest

import icp_solve_cases as CS
import icp_solve_reference as REF
from perception_amd import capi

pytestmark = pytest.mark.gpu

DRIVERS = {   # environment of the context -> cd_timing.icp_search (1: the lattice's closed form, 0: the generic searches)
    "lat": (dict(), 1),
    "sliced": (dict(CUBOID_ICP_LATTICE="0", CUBOID_ICP_MODE="sliced"), 0),
    "sliced_multi_launch": (dict(CUBOID_ICP_LATTICE="0", CUBOID_ICP_MODE="sliced", CUBOID_ICP_PERSIST="0"), 0),
    "cluster": (dict(CUBOID_ICP_LATTICE="0", CUBOID_ICP_MODE="cluster"), 0),
    "pipe": (dict(CUBOID_ICP_LATTICE="0", CUBOID_ICP_MODE="pipe"), 0),
}


@pytest.fixture(scope="module")
def scenes(template):
    """The nine scenes, each with its float64 truth (and the input assertion made)."""
    out = CS.planar_scenes(template)
    for sc in out:
        sc["want"] = REF.assert_planar_input(template, sc)
    return out


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_single_face_cluster_known_answer(driver, scenes, template, monkeypatch):
    env, search = DRIVERS[driver]
    for name in ("CUBOID_ICP_LATTICE", "CUBOID_ICP_MODE", "CUBOID_ICP_PERSIST"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = capi.Context(max_points=8192, max_frames=1)       # one context per driver, created after the environment is set
    try:
        c.set_template(0, template)
        for sc in scenes:
            who = "%s, face %d seed %d (%d points)" % (driver, sc["face"], sc["seed"], len(sc["src"]))
            prm = capi.default_params()
            prm.icp_max_iterations = 1
            st, r, _ = c.icp(0, sc["src"], prm)
            assert st == 0 and r.iterations == 1 and r.size == len(sc["src"]), who
            REF.assert_planar_first_iteration(r.T, sc["want"], who)
            st, r, _ = c.icp(0, sc["src"], capi.default_params())
            assert st == 0, who
            REF.assert_planar_converged(r, sc["want"], who)
            t = c.timing()
            assert t.icp_search == search, (who, t.icp_search, t.icp_kernel_launches)
            assert (t.icp_kernel_launches > 1) == (driver == "sliced_multi_launch"), (who, t.icp_kernel_launches)
        print("%s: icp_search %d, %d ICP launches in the last call" % (driver, t.icp_search, t.icp_kernel_launches))
    finally:
        c.close()


def test_single_face_cluster_through_the_fused_call(scenes, template):
    """Once through process_batch: each face (seed 0) above a synthetic table, one frame each, so that it arrives as a cluster."""
    sel = [sc for sc in scenes if sc["seed"] == 0]
    frames = CS.planar_table_frames(sel)
    c = capi.Context(max_points=frames.shape[1], max_frames=len(sel))
    try:
        c.set_template(0, template)
        for limit in (1, None):
            prm = CS.planar_table_params()
            if limit:
                prm.icp_max_iterations = limit
            res, _, _ = c.process_batch(frames, prm)
            for f, sc in enumerate(sel):
                who = "fused, face %d (%d points), limit %s" % (sc["face"], len(sc["src"]), limit)
                assert res[f].status == 0 and res[f].n_clusters == 1 and res[f].clusters[0].size == len(sc["src"]), who
                assert CS.same_point_set(c.cluster_points(f, 0)[:, :3], sc["src"]), who     # the cluster IS the moved face
                if limit:
                    assert res[f].clusters[0].iterations == 1, who
                    REF.assert_planar_first_iteration(res[f].clusters[0].T, sc["want"], who)
                else:
                    REF.assert_planar_converged(res[f].clusters[0], sc["want"], who)
    finally:
        c.close()
