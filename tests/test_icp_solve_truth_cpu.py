"""The single-lane ICP solve (icp_step of icp_solve.hpp, through perception_amd/csrc/icp_solve_check) and the CPU oracle's solve,
each held to a float64 Umeyama written from the definition (tests/icp_solve_reference.py) on every branch the solve can take
(tests/icp_solve_cases.py) - the rank-2 branch of single-face clusters above all, which is what production takes and which every
other ICP test only compares between the device and an oracle that restates the same lines.

For every record with a finite result, R and t taken from the outgoing T in float64:
  1. orthonormality   max |R^T R - I| <= TOL_ORTH
  2. properness       det R > 0 wherever S1 / S0 > 1e-4 (classes A-F).  For rank <= 1 the sign is REPORTED, not asserted: there
                      pcl::umeyama takes it from the float32 determinant of a singular matrix (det3(sigma) < 0 decides the sign
                      of the last column; the rank == 2 branch, the only one that looks at U and V, is not entered), and an
                      improper result is PCL's own answer (DESIGN.md, next to rule C4)
  3. optimality       |S0 + S1 + d S2 - tr(R^T sigma)| / S0 <= TOL_GAP; in class G, where R* is not unique, this and 1 are the
                      whole check of the rotation
  4. rotation         where gapmin / S0 >= 1e-3 (classes A-F): max |R - R*| <= C_ROT 2^-24 S0 / gapmin, the first-order
                      perturbation bound of the problem
  5. translation      |t_i - (mq - R mp)_i| <= 6 2^-24 (|mq_i| + sum_j |R_ij| |mp_j|): two casts, three products, three additions
  6. tail             Tfinal, iters, prev_mse, converged, done bit-equal to the restated DefaultConvergenceCriteria
TOL_ORTH, TOL_GAP and C_ROT are 4 x the oracle's own worst value over the case set, measured here (never with the code under test)."""
import os
import subprocess

import numpy as np
import pytest

import icp_solve_cases as CS
import icp_solve_reference as REF
from perception_amd import capi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "perception_amd", "csrc")
CHECK = os.path.join(CSRC, "icp_solve_check")


@pytest.fixture(scope="module")
def cases():
    return REF.with_truth(CS.case_set())


@pytest.fixture(scope="module")
def oracle_solve(O, cases):
    """(T float32 [K, 16], info list) of the oracle's float32 solve on every record."""
    out = [O.umeyama_from_moments(cases["sums"][i], int(cases["n"][i])) for i in range(len(cases["n"]))]
    return np.array([t.ravel() for t, _ in out], np.float32), [i for _, i in out]


def run_check(cases, crit, bounded, tmp_path):
    """icp_step<bounded> on every record under criteria crit (a dict of REF.criteria): (out ICP_STATE [K], done int32 [K])."""
    subprocess.run(["make", "-C", CSRC, "icp_solve_check"], check=True, stdout=subprocess.DEVNULL)
    k = len(cases["n"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([k, int(bounded), crit["max_iter"]], np.int64).tobytes())
        f.write(np.array([crit["trans_eps"], crit["rel_mse"], crit["rot_thr"], crit["abs_mse"]], np.float64).tobytes())
        f.write(cases["sums"].tobytes() + cases["n"].tobytes() + cases["states"].tobytes())
    r = subprocess.run([CHECK, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    assert len(raw) == k * (capi.ICP_STATE.itemsize + 4)
    return np.frombuffer(raw[:k * capi.ICP_STATE.itemsize], capi.ICP_STATE), np.frombuffer(raw[k * capi.ICP_STATE.itemsize:], np.int32)


def test_oracle_solve_meets_the_truth_and_sets_the_tolerances(cases, oracle_solve):
    """The oracle is held to the truth too - that is what gives "GPU == oracle" its meaning - and its worst values are the ones
    icp_solve_reference.py carries: a tolerance there is 4 x the value measured here, and a value that moved is a failure."""
    T, _ = oracle_solve
    fig, conditioned = REF.assert_solve(T, cases, "oracle")
    for name, const, sel in (("orth", REF.ORACLE_WORST_ORTH, fig["finite"]), ("gap", REF.ORACLE_WORST_GAP, fig["finite"]),
                             ("rot", REF.ORACLE_WORST_C, conditioned)):
        measured = float(fig[name][sel].max())
        assert measured <= const <= 1.01 * measured, (name, measured, const)
    assert REF.TOL_ORTH == 4 * REF.ORACLE_WORST_ORTH and REF.TOL_GAP == 4 * REF.ORACLE_WORST_GAP and REF.C_ROT == 4 * REF.ORACLE_WORST_C


def test_case_set_reaches_every_branch_and_exit(cases, oracle_solve):
    """The conditions of the case set, from the reference and the oracle's info alone."""
    cls, tr = cases["cls"], cases["truth"]
    _, info = oracle_solve
    assert len(cls) == 2500 and {c: int((cls == c).sum()) for c in CS.CLASS_SIZES} == CS.CLASS_SIZES
    for c in "ABCDEF":
        sel = cls == c
        assert (tr["gapmin"][sel] >= REF.GAP_FLOOR * tr["S"][sel, 0]).mean() >= 0.95, c
    rank = np.array([i["rank"] for i in info])
    neg = np.array([i["det_negative"] for i in info])
    uv = np.array([i["uv_positive"] for i in info])
    branches = {"rank 3, det >= 0": int(((rank == 3) & ~neg).sum()), "rank 3, det < 0": int(((rank == 3) & neg).sum()),
                "rank 2, det U det V > 0": int(((rank == 2) & uv).sum()), "rank 2, det U det V < 0": int(((rank == 2) & ~uv).sum()),
                "rank <= 1": int((rank <= 1).sum())}
    print("branches:", branches, "rank 2 per class:", {c: int(((rank == 2) & (cls == c)).sum()) for c in "ABCDEFG"})
    assert min(v for k, v in branches.items() if k != "rank <= 1") >= 50, branches
    assert ((rank == 2)[(cls == "C") | (cls == "D") | (cls == "E")]).all()      # the production branch is what C, D and E take
    exits = dict.fromkeys(REF.EXITS, 0)
    T = oracle_solve[0]
    for _, kw in CS.CRITERIA:
        for bounded in (False, True):
            for i in range(len(cls)):
                exits[REF.tail(T[i], cases["states"][i], cases["sums"][i, 15], int(cases["n"][i]), REF.criteria(**kw), bounded)[-1]] += 1
    print("exits:", exits)
    assert min(exits.values()) >= 50, exits


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("crit", CS.CRITERIA, ids=[c[0] for c in CS.CRITERIA])
def test_single_lane_step_meets_the_truth(cases, crit, bounded, tmp_path):
    """icp_step<BOUNDED> from the header the device uses: assertions 1-6."""
    c = REF.criteria(**crit[1])
    out, done = run_check(cases, c, bounded, tmp_path)
    solved = ~((cases["n"] < 3) & bounded)
    REF.assert_solve(out["T"], cases, "icp_step", solved)
    bad, exits = REF.tail_mismatches(out, done, cases["states"], cases["sums"], cases["n"], c, bounded)
    assert not bad, (len(bad), bad[:8], exits)
    assert exits["stop"] == (0 if not bounded else int((cases["n"] < 3).sum()))


def test_single_face_cluster_known_answer_on_the_oracle(O, template):
    """The CPU twin of tests/test_gpu_icp_planar_known_answer.py: a cluster that sees ONE face of the default template pairs with
    exactly coplanar template points, so the rotation comes from the rank == 2 branch; the oracle's ICP of it is held to the
    float64 Umeyama of the known pairs after one iteration, and to the inverse motion at convergence."""
    for sc in CS.planar_scenes(template):
        who = "oracle, face %d seed %d (%d points)" % (sc["face"], sc["seed"], len(sc["src"]))
        want = REF.assert_planar_input(template, sc)
        prm = capi.default_params()
        prm.icp_max_iterations = 1
        st, r, _ = O.icp(template, sc["src"], prm, nn_mode=1)
        assert st == 0 and r.iterations == 1
        REF.assert_planar_first_iteration(r.T, want, who)
        st, r, _ = O.icp(template, sc["src"], capi.default_params(), nn_mode=1)
        assert st == 0
        REF.assert_planar_converged(r, want, who)


def test_single_face_cluster_through_the_oracles_frame(O, template):
    """... and once through the whole chain, the face above a synthetic table so that it arrives as a cluster."""
    sel = [sc for sc in CS.planar_scenes(template) if sc["seed"] == 0]
    frames = CS.planar_table_frames(sel)
    for f, sc in enumerate(sel):
        want = REF.assert_planar_input(template, sc)
        for limit in (1, None):
            who = "oracle frame, face %d (%d points), limit %s" % (sc["face"], len(sc["src"]), limit)
            prm = CS.planar_table_params()
            if limit:
                prm.icp_max_iterations = limit
            r = O.process_frame(frames[f], prm, template, want_clouds=True)
            res = r["result"]
            assert r["status"] == 0 and res.status == 0 and res.n_clusters == 1 and res.n_plane == 4186, who
            assert CS.same_point_set(r["objects"][r["labels"] == 0], sc["src"]), who          # the cluster IS the moved face
            if limit:
                assert res.clusters[0].iterations == 1, who
                REF.assert_planar_first_iteration(res.clusters[0].T, want, who)
            else:
                REF.assert_planar_converged(res.clusters[0], want, who)
