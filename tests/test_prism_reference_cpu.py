"""The composed reference of a fused call with the table prism (tests/prism_reference.py), on the CPU: with the step off it is the
oracle's process_frame, and the preconditions of the GPU scenarios (tests/test_gpu_table_prism.py) hold in the reference alone."""
import numpy as np
import pytest

import prism_reference as PR
import prism_scenarios as PS
from perception_amd import capi, table_prism as TP


@pytest.fixture(scope="module")
def tpls(template):
    return {0: template}


def test_step_off_is_the_oracles_process_frame(O, template, tpls):
    frames, prm, _, keys = PS.scenario("c")
    exp = PR.expected(frames[:3], prm, tpls, keys=keys[:3])
    for rec, e in zip(frames[:3], exp):
        o = O.process_frame(rec, prm, template, want_clouds=True)
        r = o["result"]
        assert e["prism"] is None and e["outlier"] is None and len(e["hull"]) == 0
        assert (r.status, (r.n_cropped, r.n_voxels, r.n_plane, r.n_objects, r.n_clusters), r.ransac_iterations) == (e["status"], e["counts"], e["ransac_iterations"])
        assert np.array_equal(np.array(list(r.plane), np.float32), e["plane"]) and np.array_equal(o["plane_inliers"], e["plane_inliers"])
        assert np.array_equal(np.ascontiguousarray(o["objects"], np.float32).view(np.uint32).reshape(-1, 3), e["objects"][:, :3])
        assert np.array_equal(o["labels"], e["labels"]) and r.n_clusters > 0
        for k, c in enumerate(e["clusters"]):
            g = r.clusters[k]
            assert (g.size, g.iterations, g.converged, g.accepted, g.fitness) == (c.size, c.iterations, c.converged, c.accepted, c.fitness)
            assert np.array_equal(np.array(list(g.T), np.float32).reshape(4, 4), c.T)
            assert np.array_equal(np.array(list(g.pose)), c.pose)


def test_scenario_a_removes_nothing(tpls):
    frames, prm, limits, keys = PS.scenario("a")
    on = PR.expected(frames, prm, tpls, prism=limits, keys=keys)
    off = PR.expected(frames, prm, tpls, keys=keys)
    PR.same_expected(on, off)
    for e in on:
        s = e["prism"]
        assert s["n_before"] == s["n_kept"] == e["counts"][3] > 0 and (s["n_below"], s["n_above"], s["n_outside"], s["overflow"]) == (0, 0, 0, 0)
        assert 3 <= s["hull_vertices"] == len(e["hull"]) <= 64 and e["counts"][2] > 10000           # tens of vertices out of 12 - 16 k inliers
        assert (s["axis_u"], s["axis_v"]) == (0, 2)                                                   # the camera looks down at 41 degrees: y is dropped


def test_scenario_b_two_clusters_become_one(tpls):
    frames, prm, limits, keys = PS.scenario("b")
    on = PR.expected(frames, prm, tpls, prism=limits, keys=keys)
    off = PR.expected(frames, prm, tpls, keys=keys)
    for a, b in zip(off, on):
        assert a["counts"][4] == 2 and b["counts"][4] == 1
        s = b["prism"]
        assert s["n_outside"] > 1000 and (s["n_below"], s["n_above"]) == (0, 0) and s["n_kept"] == b["counts"][3]
        # the kept cluster is the one on the table, with every point it had
        heights = [TP.project(a["plane"], c.points)[0] for c in a["clusters"]]
        on_table = int(np.argmin([abs(np.median(h)) for h in heights]))
        assert np.median(heights[1 - on_table]) > 0.05
        assert np.array_equal(b["clusters"][0].points, a["clusters"][on_table].points)
        assert np.array_equal(a["plane_inliers"], b["plane_inliers"]) and np.array_equal(a["voxels"], b["voxels"])
        gated = (b["point_labels"] == capi.CD_LABEL_GATED) & (a["point_labels"] != capi.CD_LABEL_GATED)
        assert gated.sum() > 1000 and not ((b["point_labels"] != capi.CD_LABEL_GATED) & (a["point_labels"] == capi.CD_LABEL_GATED)).any()


def test_scenario_c_cuts_the_tops_off(tpls):
    frames, prm, limits, keys = PS.scenario("c")
    on = PR.expected(frames, prm, tpls, prism=limits, keys=keys)
    off = PR.expected(frames, prm, tpls, keys=keys)
    for a, b in zip(off, on):
        s = b["prism"]
        assert s["n_above"] > 0 and s["n_outside"] == 0 and s["n_kept"] == b["counts"][3] < a["counts"][3]
        assert sum(c.size for c in b["clusters"]) < sum(c.size for c in a["clusters"])


def test_prism_then_filter_composes_in_that_order(tpls):
    frames, prm, limits, keys = PS.scenario("b")
    both = PR.expected(frames[:1], prm, tpls, prism=limits, filter=(16, 1.0), keys=keys[:1])[0]
    assert both["outlier"]["n_before"] == both["prism"]["n_kept"] and both["counts"][3] == both["prism"]["n_kept"] - both["outlier"]["n_removed"]
    assert both["outlier"]["n_removed"] > 0
