"""What coarse-to-fine ICP (cd_set_icp_coarse, rule C18) does to the ICP stage.

CPU part (--cpu; the oracle and perception_amd/icp_coarse.py, no GPU), two markdown tables:
  1. object-launch parameters (leaf 0.001, plane threshold 0.01), synth.frame(0 .. --object-frames - 1), every cluster against
     each of the four scanned templates: single level against strides --object-strides at min_points --min-points - iterations
     per level, accepted pairs, point passes (sum of n (iterations + 1), the coarse level counted at its own size), the longest
     pair, the fitness ratio and the Frobenius difference of the poses;
  2. default parameters, the launch template, synth.frame(0 .. --default-frames - 1), from the rule-C13 cluster guess and from no
     guess: single level against strides --default-strides with every cluster eligible - iterations, accepted clusters, pose
     error against synth.truth_poses (minimised over the scene's boxes and the four proper flips).

GPU part (--gpu): two legs, each a child process of its own under its own time limit, the second only when the first ended well:
  object   --gpu-frames bench frames, the four scanned templates, template_slot = -1, object-launch parameters
  config3  the config-3 batch: --config3-frames bench frames, the launch template, default parameters
In a leg one context runs the fused call with the mode off and on at strides --gpu-strides (min_points --min-points), interleaved
(off, s1, s2, ..., off, s1, ...) after a warm-up of each, and prints the medians over --reps of cd_timing.stage_ms[3] and of the
wall time with the accepted and iteration totals of the batch.  No speed-up is fixed in advance: the comparison is the same
process with the mode off, whichever way it comes out.

  python tools/coarse_icp_report.py --cpu
  python tools/coarse_icp_report.py --gpu
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCANNED = ("eraser", "clamp", "screwdriver", "marker")


def scanned_templates():
    from perception_amd import pcd
    return {k: pcd.read_xyz(os.path.join(ROOT, "tests", "golden", nm + "_ascii_tf.pcd")).astype(np.float32) for k, nm in enumerate(SCANNED)}


def object_params():
    from perception_amd import capi
    prm = capi.default_params()
    prm.rgb_offset = 12
    prm.leaf_size = 0.001
    prm.plane_distance_threshold = 0.01
    return prm


def _oracle_run(O, capi, tpl, prm):
    """run(points, guess) for icp_coarse.two_level: the oracle's ICP (it has no stop: every ICP ends converged)"""
    import ctypes as C

    def run(pts, guess):
        q = capi.CdParams()
        C.memmove(C.byref(q), C.byref(prm), C.sizeof(capi.CdParams))
        q.icp_use_guess = capi.CD_GUESS_NONE
        if guess is not None:
            q.icp_use_guess = capi.CD_GUESS_PARAMS
            q.icp_guess[:] = [float(v) for v in np.asarray(guess, np.float32).ravel()]
        st, r, _ = O.icp(tpl, pts, q, nn_mode=1)
        assert st == 0
        return dict(T=np.array(list(r.T), np.float32).reshape(4, 4), iterations=r.iterations, converged=r.converged, accepted=r.accepted,
                    fitness=float(r.fitness), pose=np.array(list(r.pose)).reshape(4, 4), stopped=0)
    return run


def cpu_object_table(n_frames, strides, min_points):
    from oracle import oracle_py as O
    from perception_amd import capi, icp_coarse as IC, synth
    O.lib()
    tpls = scanned_templates()
    prm = object_params()
    rows = {s: dict(coarse=0, fine=[], acc=0, passes=0, longest=0, ratio=[], frob=[], no_worse=0) for s in [0] + list(strides)}
    sizes = []
    for i in range(n_frames):
        o = O.process_frame(synth.frame(i), prm, tpls[0], want_clouds=True)
        for k in range(o["result"].n_clusters):
            src = np.ascontiguousarray(o["objects"][o["labels"] == k])
            for slot in sorted(tpls):
                run = _oracle_run(O, capi, tpls[slot], prm)
                base = None
                sizes.append(len(src))
                for s in [0] + list(strides):
                    fine, st = IC.two_level(src, s, min_points if s else 0, run, lambda p: None)
                    row = rows[s]
                    passes = len(src) * (fine["iterations"] + 1) + st.n_coarse * (st.coarse_iterations + 1) * (st.n_coarse > 0)
                    row["coarse"] += st.coarse_iterations
                    row["fine"].append(fine["iterations"])
                    row["acc"] += int(fine["accepted"])
                    row["passes"] += passes
                    row["longest"] = max(row["longest"], passes)
                    if s == 0:
                        base = fine
                    else:
                        row["ratio"].append(fine["fitness"] / base["fitness"] if base["fitness"] > 0 else 1.0)
                        row["frob"].append(float(np.linalg.norm(fine["pose"] - base["pose"])))
                        row["no_worse"] += int(fine["fitness"] <= base["fitness"])
    n = len(sizes)
    print("CPU, object-launch parameters, synth.frame(0..%d), the four scanned templates, all pairs: %d pairs, median cluster %d points, min_points %d"
          % (n_frames - 1, n, int(np.median(sizes)), min_points))
    print("| | coarse iterations | full-res iterations (median, max) | accepted | point passes | longest pair | median fitness ratio | no worse | median / max pose difference |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in [0] + list(strides):
        r = rows[s]
        tail = "| - | - | - |" if s == 0 else "| %.3f | %d of %d | %.3g / %.3g |" % (float(np.median(r["ratio"])), r["no_worse"], n, float(np.median(r["frob"])), max(r["frob"]))
        print("| %s | %s | %d (%g, %d) | %d | %.3g (%.2fx fewer) | %.3g %s" % (
            "as today" if s == 0 else "stride %d" % s, "-" if s == 0 else "%d" % r["coarse"], sum(r["fine"]), float(np.median(r["fine"])), max(r["fine"]), r["acc"],
            r["passes"], rows[0]["passes"] / max(r["passes"], 1), r["longest"], tail))


def cpu_default_table(n_frames, strides):
    from oracle import oracle_py as O
    from perception_amd import capi, cluster_frame as cf, icp_coarse as IC, synth, templates
    O.lib()
    flips = [np.diag(f + (1.0,)) for f in cf.FLIPS]
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    t_rec = cf.shape_frame(tpl)
    prm = capi.default_params()
    run = _oracle_run(O, capi, tpl, prm)
    guess_of = {"CD_GUESS_CLUSTER": lambda p: np.asarray(cf.guess(cf.shape_frame(p), t_rec)[0], np.float32), "CD_GUESS_NONE": lambda p: None}
    rows, n_cl = {}, 0
    for i in range(n_frames):
        truths = synth.truth_poses(synth.scene_for(i))
        o = O.process_frame(synth.frame(i), prm, tpl, want_clouds=True)
        for k in range(o["result"].n_clusters):
            src = np.ascontiguousarray(o["objects"][o["labels"] == k])
            n_cl += 1
            for mode in guess_of:
                for s in [0] + list(strides):
                    fine, st = IC.two_level(src, s, 3 * s, run, guess_of[mode])
                    row = rows.setdefault((mode, s), dict(coarse=0, fine=0, acc=0, err=[]))
                    row["coarse"] += st.coarse_iterations
                    row["fine"] += fine["iterations"]
                    row["acc"] += int(fine["accepted"])
                    row["err"].append(min(float(np.linalg.norm(fine["pose"] - T @ F)) for T in truths for F in flips))
    print("\nCPU, default parameters, the launch template, synth.frame(0..%d), %d clusters, every cluster eligible (min_points = 3 stride):" % (n_frames - 1, n_cl))
    print("| guess mode | level | iterations (coarse + full-res) | accepted | median / max pose error |")
    print("|---|---|---|---|---|")
    for (mode, s), r in rows.items():
        its = "%d" % r["fine"] if s == 0 else "%d + %d" % (r["coarse"], r["fine"])
        print("| `%s` | %s | %s | %d | %.4f / %.4f |" % (mode, "as today" if s == 0 else "stride %d" % s, its, r["acc"], float(np.median(r["err"])), max(r["err"])))


def gpu_leg(leg, n_frames, strides, min_points, reps):
    """One leg, in this process: prints one markdown table."""
    from concurrent.futures import ThreadPoolExecutor
    from perception_amd import capi, synth, templates
    with ThreadPoolExecutor(16) as ex:       # (numpy releases the GIL in its array loops)
        frames = np.ascontiguousarray(np.stack(list(ex.map(synth.frame, range(n_frames)))))
    N = frames.shape[1]
    if leg == "object":
        tpls, prm = scanned_templates(), object_params()
        prm.template_slot = -1
    else:
        tpls, prm = {0: templates.template_xyz32(**templates.DEFAULT_TEMPLATE)}, capi.default_params()
        prm.rgb_offset = 12
    ctx = capi.Context(max_points=N, max_frames=n_frames)
    for slot, t in tpls.items():
        ctx.set_template(slot, t)
    settings = [0] + list(strides)

    def call(s):
        ctx.set_icp_coarse(s, min_points if s else 0)
        t0 = time.perf_counter()
        res, _, _ = ctx.process_batch(frames, prm)
        wall = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        its = acc = ncl = cits = used = 0
        for f in range(n_frames):
            for c in ctx.cluster_results(f):
                its += c.iterations
                acc += c.accepted
                ncl += 1
            if s:
                for st in ctx.cluster_coarse_stats(f):
                    cits += st.coarse_iterations
                    used += st.used == capi.CD_COARSE_USED
        return dict(wall=wall, icp=tm.stage_ms[3], total=tm.stage_ms[4], launches=tm.icp_kernel_launches, its=its, acc=acc, ncl=ncl, cits=cits, used=used)
    for s in settings:
        call(s)                                  # warm-up of each
    runs = {s: [] for s in settings}
    for _ in range(reps):
        for s in settings:
            runs[s].append(call(s))
    print("GPU, %s leg: %d bench frames, %d template(s), template_slot %d, %d clusters, min_points %d, medians of %d interleaved calls (host-fed cd_process_batch):"
          % (leg, n_frames, len(tpls), prm.template_slot, runs[0][0]["ncl"], min_points, reps))
    print("| | ICP stage ms (stage_ms[3]) | device ms (stage_ms[4]) | wall ms | ICP launches | accepted | full-res iterations | coarse iterations | pairs started from T_c |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in settings:
        r = runs[s]
        med = lambda key: float(np.median([x[key] for x in r]))
        print("| %s | %.3f | %.3f | %.2f | %d | %d | %d | %s | %s |" % ("mode off" if s == 0 else "stride %d" % s, med("icp"), med("total"), med("wall"), r[-1]["launches"],
                                                                      r[-1]["acc"], r[-1]["its"], "-" if s == 0 else r[-1]["cits"], "-" if s == 0 else r[-1]["used"]))
    ctx.close()


def gpu_part(args):
    """Each leg in a fresh child process under its own time limit; a leg that fails, faults or runs out of time ends the report."""
    for leg, n, limit in (("object", args.gpu_frames, args.object_limit), ("config3", args.config3_frames, args.config3_limit)):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-frames", str(n), "--gpu-strides", ",".join(str(s) for s in args.gpu_strides),
               "--min-points", str(args.min_points), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=limit)
        except subprocess.TimeoutExpired:
            print("the %s leg ran out of its %d s: nothing further is started" % (leg, limit))
            return 124
        if r.returncode != 0:
            print("the %s leg ended with status %d: nothing further is started" % (leg, r.returncode))
            return r.returncode
    return 0


def _ints(text):
    return [int(v) for v in text.split(",") if v]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--object-frames", type=int, default=16)
    ap.add_argument("--object-strides", type=_ints, default=[4, 16])
    ap.add_argument("--default-frames", type=int, default=32)
    ap.add_argument("--default-strides", type=_ints, default=[4, 8])
    ap.add_argument("--min-points", type=int, default=2048)
    ap.add_argument("--gpu-frames", type=int, default=64)
    ap.add_argument("--config3-frames", type=int, default=256)
    ap.add_argument("--gpu-strides", type=_ints, default=[4, 8, 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--object-limit", type=int, default=300, help="seconds the object leg may take")
    ap.add_argument("--config3-limit", type=int, default=240, help="seconds the config-3 leg may take")
    ap.add_argument("--leg", choices=("object", "config3"), default=None, help="(internal) run one GPU leg in this process")
    ap.add_argument("--leg-frames", type=int, default=64)
    args = ap.parse_args()
    if args.leg:
        gpu_leg(args.leg, args.leg_frames, args.gpu_strides, args.min_points, args.reps)
        return 0
    if args.cpu:
        cpu_object_table(args.object_frames, args.object_strides, args.min_points)
        cpu_default_table(args.default_frames, args.default_strides)
    if args.gpu:
        return gpu_part(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
