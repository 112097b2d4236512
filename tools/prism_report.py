"""What the table prism (rule C20, cd_set_table_prism) removes on the finite-table scenes, and what it costs (GPU).

Removal: the finite-table scenes of tests/prism_scenarios.py for frames [first, first + count) - the table cut to a rectangle, a
second cuboid floating beside it at 0.06 m above the plane level, crop_x widened to +-0.5 - through the fused call with the step
off and on at limits (0, 0.5).  Per frame: object points, what the step removed and why, hull vertices, clusters and accepted
poses.  The same for the project's own frames (an unbounded table), where the step should remove nothing.

Cost: a 256-frame batch of 640 x 480 records resident in HBM (synth frames 0..15 repeated), cd_process_batch_device with the
step off and on ALTERNATELY, --reps times each after warm-up calls: host wall time of the call (it ends synchronised) as
median / min / max, and the device time of stage [2] of cd_timing (extract, prism, cluster: HIP events on the context's stream).
What stage [2] gains when the step goes on is the step's one kernel and the read-back of its records.

Default path: with --bench-parent DIR (a checkout of the parent commit, built), `python bench.py --gpus 1 --steps K --warmup W`
of that tree and of this one, alternately, --bench-reps times each, every run a fresh process: the `value` of each JSON line,
median / min / max.

  timeout -k 10 900 python tools/prism_report.py --reps 10 [--bench-parent DIR --bench-reps 3]

Prints the tables and writes profiles/prism_report.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "prism_report.json")
LIMITS = (0.0, 0.5)


def removal(ctx, capi, frames, prm, tag):
    rows = []
    for on in (False, True):
        ctx.set_table_prism(on, *LIMITS)
        res, _, _ = ctx.process_batch(frames, prm)
        for f in range(len(frames)):
            r = res[f]
            nk = min(r.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)
            s = ctx.prism_stats(f) if on else None
            rows.append(dict(scene=tag, prism=int(on), frame=f, n_plane=int(r.n_plane), n_objects=int(r.n_objects), clusters=int(r.n_clusters),
                             accepted=sum(int(r.clusters[k].accepted) for k in range(nk)), sizes=[int(r.clusters[k].size) for k in range(nk)], stats=s))
    ctx.set_table_prism(False)
    return rows


def print_removal(rows):
    print("%-7s %5s %5s %8s %7s %8s %8s %8s %8s %6s %9s  %s" % ("scene", "prism", "frame", "n_plane", "n_obj", "below", "above", "outside", "clusters", "acc", "hull", "sizes"))
    for r in rows:
        s = r["stats"] or dict(n_below=0, n_above=0, n_outside=0, hull_vertices=0)
        print("%-7s %5d %5d %8d %7d %8d %8d %8d %8d %6d %9d  %s" % (r["scene"], r["prism"], r["frame"], r["n_plane"], r["n_objects"], s["n_below"], s["n_above"],
                                                                     s["n_outside"], r["clusters"], r["accepted"], s["hull_vertices"], r["sizes"]))
    summary = []
    print()
    for scene in sorted(set(r["scene"] for r in rows)):
        for on in (0, 1):
            sel = [r for r in rows if r["scene"] == scene and r["prism"] == on]
            s = dict(scene=scene, prism=on, n_objects=sum(r["n_objects"] for r in sel), clusters=sum(r["clusters"] for r in sel), accepted=sum(r["accepted"] for r in sel),
                     removed=sum(r["stats"]["n_before"] - r["stats"]["n_kept"] for r in sel) if on else 0)
            summary.append(s)
            print("%-7s prism %d: %6d object points, %5d removed, %3d clusters, %3d accepted" % (scene, on, s["n_objects"], s["removed"], s["clusters"], s["accepted"]))
    return summary


def cost(capi, torch, frames16, tpl, prm, n_frames, reps, warmup):
    big = np.ascontiguousarray(np.tile(frames16, (n_frames // len(frames16), 1, 1)))
    F, N = big.shape[:2]
    ctx = capi.Context(max_points=N, max_frames=F)
    ctx.set_template(0, tpl)
    d = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    res = (capi.CdFrameResult * F)()
    names = ("off", "on")
    wall, stage2, total = ({n: [] for n in names} for _ in range(3))
    for it in range(warmup + reps):
        for name in names:                                # alternately: the settings share whatever else the machine is doing
            ctx.set_table_prism(name == "on", *LIMITS)
            t0 = time.perf_counter()
            ctx.process_batch_device(d.data_ptr(), 16, N, F, prm, results=res)
            t1 = time.perf_counter()
            if it >= warmup:
                tm = ctx.timing()
                wall[name].append((t1 - t0) * 1e3)
                stage2[name].append(float(tm.stage_ms[2]))
                total[name].append(float(tm.stage_ms[4]))
    ctx.set_table_prism(False)
    ctx.close()
    out = {}
    fmt = lambda v: "%.3f / %.3f / %.3f" % (float(np.median(v)), min(v), max(v))
    print("%d frames of %d points, %d calls each after %d warm-up calls, alternating (ms)" % (F, N, reps, warmup))
    print("%-4s %30s %30s %30s" % ("set", "wall median / min / max", "stage [2] median / min / max", "device total median / min / max"))
    for name in names:
        print("%-4s %30s %30s %30s" % (name, fmt(wall[name]), fmt(stage2[name]), fmt(total[name])))
        out[name] = dict(wall_ms=wall[name], stage2_ms=stage2[name], device_total_ms=total[name])
    out["stage2_on_minus_off_ms"] = float(np.median(stage2["on"]) - np.median(stage2["off"]))
    out["wall_on_minus_off_ms"] = float(np.median(wall["on"]) - np.median(wall["off"]))
    print("on: stage [2] gains %.3f ms over off, the call %.3f ms" % (out["stage2_on_minus_off_ms"], out["wall_on_minus_off_ms"]))
    return out


def bench_pair(parent, reps, steps, warmup):
    """bench.py of the parent checkout and of this tree, alternately, a fresh process each: the `value` of every JSON line."""
    vals = {"parent": [], "this": []}
    for _ in range(reps):
        for name, root in (("parent", parent), ("this", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=root, capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError("bench.py of %s failed: %s" % (root, (r.stdout + r.stderr)[-2000:]))
            j = json.loads(line[-1])
            vals[name].append(float(j["value"]))
            unit = j.get("unit", "")
    for name in vals:
        print("bench.py %-6s value median / min / max: %.1f / %.1f / %.1f %s" % (name, float(np.median(vals[name])), min(vals[name]), max(vals[name]), unit))
    return dict(values=vals, unit=unit, steps=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs=2, default=(0, 16), metavar=("FIRST", "COUNT"))
    ap.add_argument("--batch", type=int, default=256, help="frames of the timed batch")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-parent", default=None, metavar="DIR", help="a built checkout of the parent commit: run its bench.py against this tree's")
    ap.add_argument("--bench-reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=10)
    args = ap.parse_args()
    bench = bench_pair(os.path.abspath(args.bench_parent), args.bench_reps, args.bench_steps, args.bench_warmup) if args.bench_parent else None
    import torch   # (before the library: one HIP runtime per process, torch's)
    import prism_scenarios as PS
    from perception_amd import capi, synth, templates
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    first, count = args.frames
    own = np.ascontiguousarray(np.stack([synth.frame(first + i) for i in range(count)]))
    finite = np.ascontiguousarray(np.stack([PS.finite_table_frame(first + i) for i in range(count)]))
    prm = capi.default_params()
    prm.rgb_offset = 12
    wide = PS.finite_table_params()
    wide.rgb_offset = 12
    ctx = capi.Context(max_points=own.shape[1], max_frames=count)
    ctx.set_template(0, tpl)
    rows = removal(ctx, capi, finite, wide, "finite") + removal(ctx, capi, own, prm, "own")
    ctx.close()
    summary = print_removal(rows)
    print()
    timing = cost(capi, torch, own, tpl, prm, args.batch, args.reps, args.warmup)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fp:
        json.dump(dict(frames=list(args.frames), limits=LIMITS, per_frame=rows, summary=summary, timing=timing, bench=bench), fp, indent=1)
    print("wrote", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    main()
