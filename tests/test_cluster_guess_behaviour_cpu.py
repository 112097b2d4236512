"""Rule C13's guess against the identity start, on the CPU with the oracle alone: every cluster of synth.frame(0..47)
(default parameters, the 7250-point default template) registered twice by O.icp - from the identity (CD_GUESS_NONE) and
from the restated guess (perception_amd.cluster_frame, handed over as CD_GUESS_PARAMS).

The three conditions are what the mode was accepted on; the figures in brackets are those of a float64 numpy prototype
(numpy.linalg.eigh, plain means), which say what to expect and are not goldens (the rule itself: 102 vs 91, 0.0043 vs 0.0611,
6103 vs 7133):
  accepted with the guess >= without                                   (102 vs 91)
  median pose error to truth with the guess <= 1/4 of the identity's   (0.0043 vs 0.061)
  total iterations with the guess <= without                           (6111 vs 7133)
Pose error = Frobenius norm of pose - truth * diag(F, 1), minimised over the scene's boxes and the four proper flips F.
No cluster is left out: there are 102 and none is merged (asserted).
"""
import numpy as np

from oracle import oracle_py as O
from perception_amd import capi, cluster_frame, synth, templates

FLIPS = [np.diag(f + (1.0,)) for f in cluster_frame.FLIPS]


def pose_error(pose, truths):
    P = np.array(pose, np.float64).reshape(4, 4)
    return min(float(np.linalg.norm(P - T @ F)) for T in truths for F in FLIPS)


def test_cluster_guess_beats_identity_on_bench_frames():
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    t_rec = cluster_frame.shape_frame(tpl)
    assert t_rec.status == 0
    prm = capi.default_params()
    acc, err, its, n_clusters = [0, 0], [[], []], [0, 0], 0
    for i in range(48):
        scene = synth.scene_for(i)
        truths = synth.truth_poses(scene)
        o = O.process_frame(synth.frame(i), prm, tpl, want_clouds=True)
        K = o["result"].n_clusters
        assert K == len(truths), "frame %d: %d clusters for %d boxes (merged or split)" % (i, K, len(truths))
        for k in range(K):
            src = o["objects"][o["labels"] == k]
            n_clusters += 1
            G, flip = cluster_frame.guess(cluster_frame.shape_frame(src), t_rec)
            assert flip >= 0
            for mode in (0, 1):
                p = capi.default_params()
                if mode:
                    p.icp_use_guess = capi.CD_GUESS_PARAMS
                    p.icp_guess[:] = [float(v) for v in G.ravel()]
                st, r, _ = O.icp(tpl, src, p)
                assert st == 0
                acc[mode] += int(r.accepted)
                its[mode] += int(r.iterations)
                err[mode].append(pose_error(r.pose, truths))
    med = [float(np.median(e)) for e in err]
    print("clusters %d" % n_clusters)
    print("accepted: identity %d, guess %d" % (acc[0], acc[1]))
    print("median pose error: identity %.6f, guess %.6f (max %.6f / %.6f)" % (med[0], med[1], max(err[0]), max(err[1])))
    print("total iterations: identity %d, guess %d" % (its[0], its[1]))
    assert n_clusters == 102
    assert acc[1] >= acc[0]
    assert med[1] <= 0.25 * med[0]
    assert its[1] <= its[0]
