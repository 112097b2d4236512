"""What reciprocal correspondences (cd_set_icp_reciprocal, rule C22) do to the ICP, and what they cost - beside the median-distance
rejector (rule C19) at --factor, on the scenes and legs of tools/reject_icp_report.py.

CPU part (--cpu; the oracle and the rules' reference pairs, tests/recip_reference.py and tests/reject_reference.py - test
infrastructure, imported from tests/ - no GPU): the contamination scene (1500 template points moved by up to 4 degrees / 8 mm with
0.7 mm noise plus a ball of 300 points 4 mm beside the object), seeds --seeds, against the launch-sized lattice template and the
eraser scan: per seed the translation error || t(T) - t(truth^-1) || in mm with the rule off, with rule C22 and with rule C19, the
iterations of each, and the correspondences rule C22 kept at its first and last iteration.  One markdown table.

GPU part (--gpu): three legs, each a child process of its own under its own time limit, the next only when the one before ended well:
  config3        the bench batch: --config3-frames bench frames, the launch template, default parameters (every ICP starts from the
                 identity, half a metre from the template)
  config3-guess  the same batch with icp_use_guess = CD_GUESS_CLUSTER (every ICP starts from rule C13's guess, on the template)
  object         --object-frames bench frames, the four scanned templates, template_slot = -1, object-launch parameters
In a leg one context runs the fused call with the default setting, with rule C19 at --factor and with rule C22, interleaved
(default, C19, C22, default, ...) after a warm-up of each, and prints what reject_icp_report.py prints: clusters, accepted, the
median and 90th percentile of the accepted poses' translation and rotation error against the nearest of synth.truth_poses, the
iteration total, the share of correspondences the last iteration kept, and the medians over --reps of cd_timing.stage_ms[3] (the
ICP stage), of the device total and of the wall time, with cd_timing.icp_kernel_launches.  The config3 legs print the same quality
figures for frames 0 .. 15 of the batch alone.  Nothing is fixed in advance: the comparison is the same process with the mode off,
whichever way it comes out.
  --leg NAME --only-recip runs one leg in this process with the default setting and rule C22 only (the form to put behind
  `rocprofv3 --kernel-trace --stats --` for the share of k_icp_recip_flags and k_icp_recip_fold among the ICP kernels).

  python tools/recip_icp_report.py --cpu
  python tools/recip_icp_report.py --gpu
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from reject_icp_report import CPU_TEMPLATES, scanned_templates   # noqa: E402  (the same scenes and templates)


def cpu_table(seeds, factor):
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import recip_reference as QR                       # (the rules' ICPs on the CPU live with the tests: the oracle is test infrastructure)
    import reject_reference as RR
    from oracle import oracle_py as O
    from perception_amd import capi, pcd
    O.lib()
    prm = capi.default_params()
    print("CPU (oracle + tests/recip_reference.py, tests/reject_reference.py), the contamination scene, default parameters:")
    print("| template | seed | error, rule off (mm) | error, reciprocal (mm) | error, C19 factor %g (mm) | iterations off / reciprocal / C19 | kept by reciprocal, first .. last iteration |" % factor)
    print("|---|---|---|---|---|---|---|")
    for name, fn in CPU_TEMPLATES:
        tpl = pcd.read_xyz(os.path.join(ROOT, "tests", "golden", fn)).astype(np.float32)
        for seed in seeds:
            src, truth = RR.contamination_scene(tpl, seed)
            st, r, _ = O.icp(tpl, src, prm, nn_mode=1)
            assert st == 0
            off = 1e3 * RR.translation_error(np.array(list(r.T), np.float64).reshape(4, 4), truth)
            q = QR.pair(tpl, src, prm)
            m = RR.pair(tpl, src, prm, factor)
            print("| %s | %d | %.2f | %.2f | %.2f | %d / %d / %d | %d .. %d |" % (
                name, seed, off, 1e3 * RR.translation_error(q["T"], truth), 1e3 * RR.translation_error(m["T"], truth), r.iterations, q["iterations"], m["iterations"],
                q["kept"][0], q["kept"][-1]))


def gpu_leg(leg, n_frames, factor, reps, only_recip=False):
    """One leg, in this process: prints markdown tables."""
    from concurrent.futures import ThreadPoolExecutor
    from perception_amd import capi, synth, templates
    from verify_report import pose_error
    with ThreadPoolExecutor(16) as ex:       # (numpy releases the GIL in its array loops)
        frames = np.ascontiguousarray(np.stack(list(ex.map(synth.frame, range(n_frames)))))
    truths = [synth.truth_poses(synth.scene_for(i)) for i in range(n_frames)]
    N = frames.shape[1]
    prm = capi.default_params()
    prm.rgb_offset = 12
    if leg == "config3-guess":
        prm.icp_use_guess = capi.CD_GUESS_CLUSTER
    if leg == "object":
        tpls = scanned_templates()
        prm.leaf_size = 0.001
        prm.plane_distance_threshold = 0.01
        prm.template_slot = -1
    else:
        tpls = {0: templates.template_xyz32(**templates.DEFAULT_TEMPLATE)}
    ctx = capi.Context(max_points=N, max_frames=n_frames)
    for slot, t in tpls.items():
        ctx.set_template(slot, t)
    settings = [("default", 0.0, False)]
    if not only_recip:
        settings.append(("C19 factor %g" % factor, factor, False))
    settings.append(("C22 reciprocal", 0.0, True))

    def call(setting):
        _, f, recip = setting
        ctx.set_icp_median_rejection(f)
        ctx.set_icp_reciprocal(recip)
        t0 = time.perf_counter()
        ctx.process_batch(frames, prm)
        wall = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        rows = []
        for fr in range(n_frames):
            stats = ctx.cluster_recip_stats(fr) if recip else (ctx.cluster_reject_stats(fr) if f else None)
            for k, c in enumerate(ctx.cluster_results(fr)):
                mm, deg, _ = pose_error(c.pose, truths[fr]) if c.accepted and truths[fr] else (None, None, None)
                rows.append(dict(frame=fr, its=c.iterations, acc=c.accepted, mm=mm, deg=deg, size=c.size,
                                 share=(stats[k].last_kept / c.size) if stats is not None and c.size else None))
        return dict(wall=wall, icp=tm.stage_ms[3], total=tm.stage_ms[4], launches=tm.icp_kernel_launches, rows=rows)
    for s in settings:
        call(s)                                  # warm-up of each
    runs = {s[0]: [] for s in settings}
    for _ in range(reps):
        for s in settings:
            runs[s[0]].append(call(s))

    def quality(first_frames):
        print("| | clusters | accepted | translation error mm (median / p90) | rotation error deg (median / p90) | iterations | kept by the last iteration (median) |")
        print("|---|---|---|---|---|---|---|")
        for name, _, _ in settings:
            rows = [r for r in runs[name][-1]["rows"] if r["frame"] < first_frames]
            mm = [r["mm"] for r in rows if r["mm"] is not None]
            deg = [r["deg"] for r in rows if r["deg"] is not None]
            pct = lambda v, q: float(np.percentile(v, q)) if v else float("nan")
            share = [r["share"] for r in rows if r["share"] is not None]
            print("| %s | %d | %d | %.2f / %.2f | %.3f / %.3f | %d | %s |" % (name, len(rows), sum(r["acc"] for r in rows), pct(mm, 50), pct(mm, 90), pct(deg, 50), pct(deg, 90),
                                                                        sum(r["its"] for r in rows), "%.0f %%" % (100 * float(np.median(share))) if share else "-"))
    print("GPU, %s leg: %d bench frames, %d template(s), template_slot %d, medians of %d interleaved calls (host-fed cd_process_batch):"
          % (leg, n_frames, len(tpls), prm.template_slot, reps))
    quality(n_frames)
    if leg != "object" and n_frames > 16:
        print("\nthe same calls, frames 0 .. 15 alone:")
        quality(16)
    print("\n| | ICP stage ms (stage_ms[3]) | device ms (stage_ms[4]) | wall ms | ICP launches |")
    print("|---|---|---|---|---|")
    for name, _, _ in settings:
        r = runs[name]
        med = lambda key: float(np.median([x[key] for x in r]))
        print("| %s | %.3f | %.3f | %.2f | %d |" % (name, med("icp"), med("total"), med("wall"), r[-1]["launches"]))
    print()
    sys.stdout.flush()
    ctx.close()


def gpu_part(args):
    """Each leg in a fresh child process under its own time limit; a leg that fails, faults or runs out of time ends the report."""
    for leg, n, limit in (("config3", args.config3_frames, args.config3_limit), ("config3-guess", args.config3_frames, args.config3_limit),
                          ("object", args.object_frames, args.object_limit)):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--leg-frames", str(n), "--factor", "%g" % args.factor, "--reps", str(args.reps)]
        sys.stdout.flush()
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
    ap.add_argument("--seeds", type=_ints, default=[2, 3, 4, 5])
    ap.add_argument("--factor", type=float, default=4.0, help="rule C19's factor in the comparison")
    ap.add_argument("--config3-frames", type=int, default=256)
    ap.add_argument("--object-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config3-limit", type=int, default=300, help="seconds a config-3 leg may take")
    ap.add_argument("--object-limit", type=int, default=420, help="seconds the object leg may take")
    ap.add_argument("--leg", choices=("config3", "config3-guess", "object"), default=None, help="run one GPU leg in this process")
    ap.add_argument("--leg-frames", type=int, default=None)
    ap.add_argument("--only-recip", action="store_true", help="with --leg: the default setting and rule C22 only")
    args = ap.parse_args()
    if args.leg:
        n = args.leg_frames or (args.object_frames if args.leg == "object" else args.config3_frames)
        gpu_leg(args.leg, n, args.factor, args.reps, only_recip=args.only_recip)
        return 0
    if args.cpu:
        cpu_table(args.seeds, args.factor)
    if args.gpu:
        return gpu_part(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
