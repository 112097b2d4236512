"""What the plane-weighted ICP step (cd_set_icp_plane_weight, rule C17) does to the ICP.

CPU part (always; the oracle and perception_amd/icp_plane.py, no GPU): every cluster of synth.frame(0 .. --cpu-frames - 1)
(default parameters, the launch template) registered by the oracle's point-to-point ICP and by the module at --weight /
--switch, from the identity and from the rule-C13 cluster guess -> accepted clusters, total iterations, pose error against
synth.truth_poses (Frobenius norm, minimised over the scene's boxes and the four proper flips); one markdown table.

GPU part (when a context can be created): one context, one batch of --frames synth frames (the bench workload), the fused call
with the mode off and on in the SAME process, interleaved (off, on, off, on, ...) after a warm-up of both, medians over --reps:
wall ms per batch, device ms per batch (cd_timing.stage_ms[4]), ICP stage ms (stage_ms[3]), and the ICP iteration and accepted
totals of the batch - once with icp_use_guess = CD_GUESS_NONE and once with CD_GUESS_CLUSTER.  No time is fixed in advance: the
comparison is the ICP stage with the mode on against the mode off, whichever way it comes out.

  timeout -k 10 900 python tools/icp_plane_report.py
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cpu_table(n_frames, weight, switch):
    from oracle import oracle_py as O
    from perception_amd import capi, cluster_frame as cf, icp_plane as IP, synth, templates
    flips = [np.diag(f + (1.0,)) for f in cf.FLIPS]
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    axes = IP.face_axes(tpl)
    t_rec = cf.shape_frame(tpl)
    prm = capi.default_params()
    rows = {}
    n_cl = 0
    for i in range(n_frames):
        truths = synth.truth_poses(synth.scene_for(i))
        o = O.process_frame(synth.frame(i), prm, tpl, want_clouds=True)
        for k in range(o["result"].n_clusters):
            src = o["objects"][o["labels"] == k]
            n_cl += 1
            G = np.asarray(cf.guess(cf.shape_frame(src), t_rec)[0], np.float32)
            for start, guess in (("identity", None), ("C13 cluster guess", G)):
                p = capi.default_params()
                if guess is not None:
                    p.icp_use_guess = capi.CD_GUESS_PARAMS
                    p.icp_guess[:] = [float(v) for v in guess.ravel()]
                _, r, _ = O.icp(tpl, src, p)
                m = IP.icp(tpl, axes, src, prm, weight, switch, guess=guess)
                Tm = m.T.astype(np.float64)
                for step, acc, its, pose, sing in (("point-to-point (oracle)", r.accepted, r.iterations, np.array(r.pose).reshape(4, 4), 0),
                                                   ("plane-weighted", m.accepted, m.iterations, np.linalg.inv(Tm), m.stopped_singular)):
                    row = rows.setdefault((start, step), dict(acc=0, its=0, err=[], sing=0))
                    row["acc"] += int(acc)
                    row["its"] += int(its)
                    row["sing"] += int(sing)
                    row["err"].append(min(float(np.linalg.norm(pose - T @ F)) for T in truths for F in flips))
    print("CPU (oracle + perception_amd/icp_plane.py), synth.frame(0..%d), %d clusters, tangent_weight %g, switch_distance %g:" % (n_frames - 1, n_cl, weight, switch))
    print("| start | step | accepted | total iterations | median pose error (Frobenius) | max | singular stops |")
    print("|---|---|---|---|---|---|---|")
    for (start, step), row in rows.items():
        print("| %s | %s | %d / %d | %d | %.4f | %.4f | %d |" % (start, step, row["acc"], n_cl, row["its"], np.median(row["err"]), max(row["err"]), row["sing"]))


def gpu_part(n_frames, reps, weight, switch):
    from perception_amd import capi, synth, templates
    from concurrent.futures import ThreadPoolExecutor
    try:
        ctx = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=n_frames)
    except capi.CuboidError:
        print("GPU part skipped: no context (no usable HIP device)")
        return
    try:
        with ThreadPoolExecutor(16) as ex:
            frames = np.stack(list(ex.map(synth.frame, range(n_frames))), 0)
        ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
        settings = [(0.0, switch), (weight, switch)]
        for guess_name, guess_mode in (("CD_GUESS_NONE", capi.CD_GUESS_NONE), ("CD_GUESS_CLUSTER", capi.CD_GUESS_CLUSTER)):
            prm = capi.default_params()
            prm.icp_use_guess = guess_mode
            wall, dev, icp = [[], []], [[], []], [[], []]
            totals = [None, None]
            for mode in (0, 1, 0, 1):   # warm-up: both settings, twice (buffers grown, clocks up)
                ctx.set_icp_plane_weight(*settings[mode])
                ctx.process_batch(frames, prm)
            for _ in range(reps):
                for mode in (0, 1):
                    ctx.set_icp_plane_weight(*settings[mode])
                    t0 = time.perf_counter()
                    ctx.process_batch(frames, prm)
                    wall[mode].append((time.perf_counter() - t0) * 1e3)
                    t = ctx.timing()
                    dev[mode].append(float(t.stage_ms[4]))
                    icp[mode].append(float(t.stage_ms[3]))
                    if totals[mode] is None:
                        n_cl = its = acc = plane_its = sing = 0
                        for f in range(n_frames):
                            for c in ctx.cluster_results(f):
                                n_cl += 1
                                its += c.iterations
                                acc += c.accepted
                            if mode:
                                s = ctx.cluster_plane_stats(f)
                                plane_its += int(s[:, 0].sum())
                                sing += int(s[:, 2].sum())
                        totals[mode] = (n_cl, its, acc, plane_its, sing)
            print("GPU, one context, one batch of %d synth frames, host-fed fused call, %s, interleaved, medians of %d:" % (n_frames, guess_name, reps))
            print("| plane weight | wall ms / batch | device ms / batch | ICP stage ms | clusters | ICP iterations | accepted | plane iterations | singular stops |")
            print("|---|---|---|---|---|---|---|---|---|")
            for mode, name in ((0, "off"), (1, "(%g, %g)" % (weight, switch))):
                print("| %s | %.2f | %.2f | %.2f | %d | %d | %d | %d | %d |" % ((name, np.median(wall[mode]), np.median(dev[mode]), np.median(icp[mode])) + totals[mode]))
            print("spread (min .. max) of ICP stage ms: off %.2f .. %.2f, on %.2f .. %.2f" % (min(icp[0]), max(icp[0]), min(icp[1]), max(icp[1])))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu-frames", type=int, default=16, help="frames of the CPU table (0: skip it)")
    ap.add_argument("--frames", type=int, default=256, help="frames of the GPU batch (0: skip the GPU part)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--weight", type=float, default=1.0 / 32.0)
    ap.add_argument("--switch", type=float, default=0.01)
    args = ap.parse_args()
    if args.cpu_frames > 0:
        cpu_table(args.cpu_frames, args.weight, args.switch)
    if args.frames > 0:
        gpu_part(args.frames, args.reps, args.weight, args.switch)


if __name__ == "__main__":
    main()
