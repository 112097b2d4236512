"""What the per-cluster principal-frame guess (icp_use_guess = CD_GUESS_CLUSTER, rule C13) does to the ICP.

CPU part (always; the oracle and perception_amd/cluster_frame.py, no GPU): every cluster of synth.frame(0 .. --cpu-frames - 1)
(default parameters, the launch template) registered by the oracle from the identity and from the restated guess -> accepted
clusters, pose error against synth.truth_poses (Frobenius norm, minimised over the scene's boxes and the four proper flips),
fitness, iterations; one markdown table.

GPU part (when a context can be created): one context, one batch of --frames synth frames (the bench workload), the fused call
with CD_GUESS_NONE and with CD_GUESS_CLUSTER in the SAME process, interleaved (none, cluster, none, cluster, ...) after a warm-up
of both, medians over --reps: wall ms per batch, device ms per batch (cd_timing.stage_ms[4]), ICP stage ms, and the ICP iteration
and accepted totals of the batch.

  timeout -k 10 600 python tools/cluster_guess_report.py
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cpu_table(n_frames):
    from oracle import oracle_py as O
    from perception_amd import capi, cluster_frame as cf, synth, templates
    flips = [np.diag(f + (1.0,)) for f in cf.FLIPS]
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    t_rec = cf.shape_frame(tpl)
    prm = capi.default_params()
    acc, its, err, fit, n_cl, worse = [0, 0], [0, 0], [[], []], [[], []], 0, 0
    for i in range(n_frames):
        truths = synth.truth_poses(synth.scene_for(i))
        o = O.process_frame(synth.frame(i), prm, tpl, want_clouds=True)
        for k in range(o["result"].n_clusters):
            src = o["objects"][o["labels"] == k]
            n_cl += 1
            G, _ = cf.guess(cf.shape_frame(src), t_rec)
            pair = []
            for mode in (0, 1):
                p = capi.default_params()
                if mode:
                    p.icp_use_guess = capi.CD_GUESS_PARAMS
                    p.icp_guess[:] = [float(v) for v in G.ravel()]
                _, r, _ = O.icp(tpl, src, p)
                P = np.array(r.pose).reshape(4, 4)
                acc[mode] += int(r.accepted)
                its[mode] += int(r.iterations)
                err[mode].append(min(float(np.linalg.norm(P - T @ F)) for T in truths for F in flips))
                fit[mode].append(float(r.fitness))
                pair.append(float(r.fitness))
            worse += int(pair[1] > pair[0])
    print("CPU (oracle + restatement), synth.frame(0..%d), %d clusters:" % (n_frames - 1, n_cl))
    print("| per-cluster ICP start | accepted | median pose error | max | median fitness | total iterations |")
    print("|---|---|---|---|---|---|")
    for mode, name in ((0, "identity"), (1, "principal-frame guess")):
        print("| %s | %d / %d | %.4f | %.4f | %.2g | %d |" % (name, acc[mode], n_cl, np.median(err[mode]), max(err[mode]),
                                                            np.median(fit[mode]), its[mode]))
    print("clusters whose fitness is worse with the guess: %d" % worse)


def gpu_part(n_frames, reps):
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
        prms = [capi.default_params(), capi.default_params()]
        prms[1].icp_use_guess = capi.CD_GUESS_CLUSTER
        wall, dev, icp = [[], []], [[], []], [[], []]
        totals = [None, None]
        for mode in (0, 1, 0, 1):   # warm-up: both modes, twice (buffers grown, clocks up)
            ctx.process_batch(frames, prms[mode])
        for _ in range(reps):
            for mode in (0, 1):
                t0 = time.perf_counter()
                res, _, _ = ctx.process_batch(frames, prms[mode])
                wall[mode].append((time.perf_counter() - t0) * 1e3)
                t = ctx.timing()
                dev[mode].append(float(t.stage_ms[4]))
                icp[mode].append(float(t.stage_ms[3]))
                if totals[mode] is None:
                    n_cl = its = acc = flagged = 0
                    for f in range(n_frames):
                        for c in ctx.cluster_results(f):
                            n_cl += 1
                            its += c.iterations
                            acc += c.accepted
                        flagged += 1 if res[f].flags & capi.CD_FRAME_CLUSTER_GUESS else 0
                    totals[mode] = (n_cl, its, acc, flagged)
        print("GPU, one context, one batch of %d synth frames, host-fed fused call, interleaved, medians of %d:" % (n_frames, reps))
        print("| icp_use_guess | wall ms / batch | device ms / batch | ICP stage ms | clusters | ICP iterations | accepted | frames flagged |")
        print("|---|---|---|---|---|---|---|---|")
        for mode, name in ((0, "CD_GUESS_NONE"), (1, "CD_GUESS_CLUSTER")):
            print("| %s | %.2f | %.2f | %.2f | %d | %d | %d | %d |" % ((name, np.median(wall[mode]), np.median(dev[mode]), np.median(icp[mode])) + totals[mode]))
        print("spread (min .. max) of device ms: none %.2f .. %.2f, cluster %.2f .. %.2f" % (min(dev[0]), max(dev[0]), min(dev[1]), max(dev[1])))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu-frames", type=int, default=48, help="frames of the CPU table (0: skip it)")
    ap.add_argument("--frames", type=int, default=256, help="frames of the GPU batch (0: skip the GPU part)")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if args.cpu_frames > 0:
        cpu_table(args.cpu_frames)
    if args.frames > 0:
        gpu_part(args.frames, args.reps)


if __name__ == "__main__":
    main()
