"""What the statistical outlier filter (rule C16, cd_set_outlier_filter) does to the project's own frames, and what it costs (GPU).

Quality: synth frames [first, first + count), clean and with synth.flying_pixels (seed 7, frac 0.5), each batch through the
fused call with the filter off and on at (mean_k, std_mul) = (16, 1.0) and (50, 1.0).  Per frame: points the filter removed,
clusters, accepted poses, the fitness of the largest cluster, and the pose error of the accepted poses against the nearest of
synth.truth_poses (translation in mm, rotation in degrees, minimised over the cuboid's 180-degree turns; the worst of the frame).

Cost: a 256-frame batch of 640 x 480 records resident in HBM (the 16 clean frames repeated), cd_process_batch_device with the
filter off and on ALTERNATELY, --reps times each after warm-up calls: host wall time of the call (it ends synchronised) as
median / min / max, and the device time of stage [2] of cd_timing (extract, filter, cluster: HIP events on the context's
stream).  The filter's own kernels are what stage [2] gains when the filter goes on - less what the smaller clouds save the
clustering - and that difference is reported as such.

  timeout -k 10 900 python tools/outlier_filter_report.py --reps 10

Prints the tables and writes profiles/outlier_filter_report.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "outlier_filter_report.json")
SETTINGS = [("off", 0, 1.0), ("k16", 16, 1.0), ("k50", 50, 1.0)]


def quality(ctx, capi, synth, frames, scenes, prm, tag):
    from verify_report import pose_error
    rows = []
    for name, mean_k, std_mul in SETTINGS:
        ctx.set_outlier_filter(mean_k, std_mul)
        res, _, _ = ctx.process_batch(frames, prm)
        for f in range(len(frames)):
            r = res[f]
            truths = synth.truth_poses(scenes[f])
            nk = min(r.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)
            acc = [r.clusters[k] for k in range(nk) if r.clusters[k].accepted]
            errs = [pose_error(c.pose, truths)[:2] for c in acc]
            rows.append(dict(cloud=tag, setting=name, frame=f, n_objects=int(r.n_objects),
                             removed=int(ctx.outlier_stats(f)["n_removed"]) if mean_k else 0,
                             clusters=int(r.n_clusters), accepted=len(acc),
                             fitness=float(r.clusters[0].fitness) if nk else None,
                             err_mm=max((e[0] for e in errs), default=None), err_deg=max((e[1] for e in errs), default=None)))
    ctx.set_outlier_filter(0)
    return rows


def print_quality(rows):
    print("%-6s %-4s %5s %7s %7s %8s %8s %11s %8s %8s" % ("cloud", "set", "frame", "n_obj", "removed", "clusters", "accepted", "fitness", "err_mm", "err_deg"))
    for r in rows:
        print("%-6s %-4s %5d %7d %7d %8d %8d %11s %8s %8s" % (
            r["cloud"], r["setting"], r["frame"], r["n_objects"], r["removed"], r["clusters"], r["accepted"],
            "%.3e" % r["fitness"] if r["fitness"] is not None else "-",
            "%.3f" % r["err_mm"] if r["err_mm"] is not None else "-", "%.4f" % r["err_deg"] if r["err_deg"] is not None else "-"))
    print()
    print("%-6s %-4s %9s %9s %9s %12s %10s %10s" % ("cloud", "set", "removed", "clusters", "accepted", "med fitness", "med mm", "med deg"))
    summary = []
    for cloud in ("clean", "flying"):
        for name, _, _ in SETTINGS:
            sel = [r for r in rows if r["cloud"] == cloud and r["setting"] == name]
            med = lambda key: float(np.median([r[key] for r in sel if r[key] is not None])) if any(r[key] is not None for r in sel) else None
            s = dict(cloud=cloud, setting=name, removed=sum(r["removed"] for r in sel), clusters=sum(r["clusters"] for r in sel),
                     accepted=sum(r["accepted"] for r in sel), fitness=med("fitness"), err_mm=med("err_mm"), err_deg=med("err_deg"))
            summary.append(s)
            nan = float("nan")
            print("%-6s %-4s %9d %9d %9d %12.3e %10.3f %10.4f" % (cloud, name, s["removed"], s["clusters"], s["accepted"],
                                                                  s["fitness"] if s["fitness"] is not None else nan,
                                                                  s["err_mm"] if s["err_mm"] is not None else nan, s["err_deg"] if s["err_deg"] is not None else nan))
    return summary


def cost(capi, torch, frames16, tpl, prm, n_frames, reps, warmup):
    reps_of = n_frames // len(frames16)
    big = np.ascontiguousarray(np.tile(frames16, (reps_of, 1, 1)))
    F, N = big.shape[:2]
    ctx = capi.Context(max_points=N, max_frames=F)
    ctx.set_template(0, tpl)
    d = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    res = (capi.CdFrameResult * F)()
    wall = {name: [] for name, _, _ in SETTINGS}
    stage2 = {name: [] for name, _, _ in SETTINGS}
    total = {name: [] for name, _, _ in SETTINGS}
    for it in range(warmup + reps):
        for name, mean_k, std_mul in SETTINGS:           # alternately: the settings share whatever else the machine is doing
            ctx.set_outlier_filter(mean_k, std_mul)
            t0 = time.perf_counter()
            ctx.process_batch_device(d.data_ptr(), 16, N, F, prm, results=res)
            t1 = time.perf_counter()
            if it >= warmup:
                tm = ctx.timing()
                wall[name].append((t1 - t0) * 1e3)
                stage2[name].append(float(tm.stage_ms[2]))
                total[name].append(float(tm.stage_ms[4]))
    ctx.set_outlier_filter(0)
    ctx.close()
    out = {}
    print("%d frames of %d points, %d calls each after %d warm-up calls, alternating (ms)" % (F, N, reps, warmup))
    print("%-4s %30s %30s %30s" % ("set", "wall median / min / max", "stage [2] median / min / max", "device total median / min / max"))
    for name, _, _ in SETTINGS:
        fmt = lambda v: "%.3f / %.3f / %.3f" % (float(np.median(v)), min(v), max(v))
        print("%-4s %30s %30s %30s" % (name, fmt(wall[name]), fmt(stage2[name]), fmt(total[name])))
        out[name] = dict(wall_ms=wall[name], stage2_ms=stage2[name], device_total_ms=total[name])
    for name in ("k16", "k50"):
        d2 = float(np.median(stage2[name]) - np.median(stage2["off"]))
        dw = float(np.median(wall[name]) - np.median(wall["off"]))
        out[name]["stage2_minus_off_ms"] = d2
        out[name]["wall_minus_off_ms"] = dw
        print("%s: stage [2] gains %.3f ms over off (the filter's two kernels less what clustering saves), the call %.3f ms" % (name, d2, dw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs=2, default=(0, 16), metavar=("FIRST", "COUNT"))
    ap.add_argument("--batch", type=int, default=256, help="frames of the timed batch")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch   # (before the library: one HIP runtime per process, torch's)
    from perception_amd import capi, synth, templates
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = capi.default_params()
    prm.rgb_offset = 12
    first, count = args.frames
    scenes = [synth.scene_for(first + i) for i in range(count)]
    clean = np.ascontiguousarray(np.stack([synth.frame(first + i) for i in range(count)]))
    flying = np.ascontiguousarray(np.stack([synth.flying_pixels(clean[i], synth.WIDTH, synth.HEIGHT, seed=7, frac=0.5) for i in range(count)]))
    ctx = capi.Context(max_points=clean.shape[1], max_frames=count)
    ctx.set_template(0, tpl)
    rows = quality(ctx, capi, synth, clean, scenes, prm, "clean") + quality(ctx, capi, synth, flying, scenes, prm, "flying")
    ctx.close()
    summary = print_quality(rows)
    print()
    timing = cost(capi, torch, clean, tpl, prm, args.batch, args.reps, args.warmup)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fp:
        json.dump(dict(frames=list(args.frames), settings=SETTINGS, per_frame=rows, summary=summary, timing=timing), fp, indent=1)
    print("wrote", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    main()
