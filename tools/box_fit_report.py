"""What the box fit (cd_set_box_fit, rule C24) measures against the synthetic truth, and what it costs.  GPU.

Four legs, each a child process of its own under its own time limit, the next only when the one before ended well:
  synth    synth.frame(0 .. --synth-frames - 1), the launch template, default parameters, the step on at the default band: for every
           cluster the errors of L, W, H, the centre and the long axis against the box of synth.truth_poses nearest its centroid,
           next to the accepted ICP poses' translation error on the same clusters.
  config5  --config5-scenes scenes of synth.scene_config5 rendered at 640 x 480 with config 5's crops and its five templates,
           template_slot = -1: the same errors, and cd_box_fit_match's slot (tolerance 0.0125) against the true box and against the
           slot the all-pairs ICP kept.  Then the same call with nothing set, with the box fit alone and with the selection
           (cd_set_box_select), ALTERNATELY, --reps times each after a warm-up of each: the ICP stage, the device total, the wall
           time and the ICP pair tests, and how many clusters report their true slot.
  worst    the kernel's worst cases as cd_box_fit_points calls of one set: a hull at the cap of 1024 vertices with 0, 5 000 and
           50 000 further points inside it (the march reads every point once per hull vertex; beyond CD_BOX_FIT_LDS_POINTS it
           quantises them again each time), wall time of the call, the median of --reps.
  cost     --cost-frames bench frames, the launch template, default parameters: one context runs the fused call (host-fed
           cd_process_batch) with the step off and on ALTERNATELY, --reps times each after a warm-up of each, and prints the medians,
           minima and maxima of cd_timing.stage_ms[3] (the stage the step's launch is part of: on minus off is what the step costs),
           of the device total and of the wall time.

  python tools/box_fit_report.py
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

TOLERANCE = 0.0125


def frames_of(n):
    from concurrent.futures import ThreadPoolExecutor
    from perception_amd import synth
    with ThreadPoolExecutor(16) as ex:       # (numpy releases the GIL in its array loops)
        return np.ascontiguousarray(np.stack(list(ex.map(synth.frame, range(n)))))


def errors(rec, box):
    """(dL, dW, dH, centre distance, axis error in degrees) of a record against a truth box (R, c, half: box -> camera)."""
    dims = 2.0 * box["half"]
    L, W = max(dims[0], dims[1]), min(dims[0], dims[1])
    P = np.array(list(rec.pose), np.float64).reshape(4, 4)
    tx = box["R"][:, 0] if dims[0] >= dims[1] else box["R"][:, 1]
    yaw = np.degrees(np.arccos(min(1.0, abs(float(P[:3, 0] @ tx)))))       # (an axis: the box is symmetric under a half turn)
    return rec.dims[0] - L, rec.dims[1] - W, rec.dims[2] - dims[2], float(np.linalg.norm(P[:3, 3] - box["c"])), yaw


def table(rows, icp_err):
    E = np.array(rows)
    print("| quantity | min | median | max |")
    print("|---|---|---|---|")
    for j, (name, scale, unit) in enumerate((("dL", 1e3, "mm"), ("dW", 1e3, "mm"), ("dH", 1e3, "mm"), ("centre error", 1e3, "mm"), ("long-axis error", 1.0, "deg"))):
        print("| %s (%s) | %.2f | %.2f | %.2f |" % (name, unit, scale * E[:, j].min(), scale * float(np.median(E[:, j])), scale * E[:, j].max()))
    if len(icp_err):
        print("| accepted ICP poses' translation error (mm), %d results | %.2f | %.2f | %.2f |" % (len(icp_err), 1e3 * min(icp_err), 1e3 * float(np.median(icp_err)),
                                                                                               1e3 * max(icp_err)))


def collect(ctx, scenes, match=None):
    """Per cluster of the last fused call: the record's errors against the nearest truth box, the ICP pose's translation error when
    accepted, and (match = slot dims) the matched slot with its cost, the true box and the slot the ICP kept."""
    rows, icp_err, picks, bad = [], [], [], 0
    for f, sc in enumerate(scenes):
        res, fits = ctx.cluster_results(f), ctx.cluster_box_fits(f)
        for k, (r, b) in enumerate(zip(res, fits)):
            pts = ctx.cluster_points(f, k, aligned=False)[:, :3]
            i = int(np.argmin([np.linalg.norm(pts.mean(axis=0) - bx["c"]) for bx in sc["boxes"]]))
            if b.status != 0:
                bad += 1
                continue
            rows.append(errors(b, sc["boxes"][i]))
            if r.accepted:
                icp_err.append(float(np.linalg.norm(np.array(list(r.pose)).reshape(4, 4)[:3, 3] - sc["boxes"][i]["c"])))
            if match is not None:
                from perception_amd import capi
                picks.append(capi.box_fit_match(list(b.dims), match, (1 << len(match)) - 1, TOLERANCE) + (i, r.template_slot))
    return rows, icp_err, picks, bad


def synth_leg(n_frames):
    from perception_amd import capi, synth, templates
    frames = frames_of(n_frames)
    prm = capi.default_params()
    prm.rgb_offset = 12
    ctx = capi.Context(max_points=frames.shape[1], max_frames=n_frames)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    ctx.set_box_fit(True)
    ctx.process_batch(frames, prm)
    rows, icp_err, _, bad = collect(ctx, [synth.scene_for(f) for f in range(n_frames)])
    ctx.close()
    print("GPU, synth.frame(0..%d), the launch template, band %g: %d clusters with a box record, %d without" % (n_frames - 1, capi.CD_BOX_FIT_BAND_DEFAULT, len(rows), bad))
    table(rows, icp_err)
    print()


def config5_leg(n_scenes, reps):
    from perception_amd import capi, synth, templates
    scenes = [synth.scene_config5(i) for i in range(n_scenes)]
    frames = np.ascontiguousarray(np.stack([synth.render(sc, width=640, height=480) for sc in scenes]))
    prm = capi.default_params()
    prm.rgb_offset = 12
    prm.crop_x_min, prm.crop_x_max = -synth.CONFIG5_CROP_X, synth.CONFIG5_CROP_X
    prm.crop_z_max = prm.crop2_z_max = 1.2
    prm.template_slot = -1
    ctx = capi.Context(max_points=frames.shape[1], max_frames=n_scenes)
    for slot, (L, W, H, d) in enumerate(synth.CONFIG5_DIMS):
        ctx.set_template(slot, templates.template_xyz32(L, W, H, d))
    ctx.set_box_fit(True)
    ctx.process_batch(frames, prm)
    dims = [d[:3] for d in synth.CONFIG5_DIMS]
    rows, icp_err, picks, bad = collect(ctx, scenes, match=dims)
    pairs = ctx.timing()
    print("GPU, synth.scene_config5(0..%d) at 640 x 480, five templates, template_slot = -1: %d clusters with a box record, %d without" % (n_scenes - 1, len(rows), bad))
    table(rows, icp_err)
    true_cost = [c for s, c, i, _ in picks if s == i]
    print("cd_box_fit_match (tolerance %g) names the true box for %d of %d clusters (worst cost of those %.2f mm); the all-pairs ICP kept the true slot for %d of %d; "
          "the call made %d ICP pair tests\n" % (TOLERANCE, sum(1 for s, _, i, _ in picks if s == i), len(picks), 1e3 * max(true_cost or [0.0]),
                                              sum(1 for _, _, i, t in picks if t == i), len(picks),
                                              (pairs.icp_pair_tests_hi << 32) | (pairs.icp_pair_tests_lo & 0xffffffff)))

    def call(mode):
        ctx.set_box_fit(mode != "off")
        ctx.set_box_select(mode == "select", dims, TOLERANCE)
        t0 = time.perf_counter()
        ctx.process_batch(frames, prm)
        wall = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        true_slot = sum(1 for f, sc in enumerate(scenes) for k, r in enumerate(ctx.cluster_results(f))
                        if r.template_slot == int(np.argmin([np.linalg.norm(ctx.cluster_points(f, k)[:, :3].mean(axis=0) - bx["c"]) for bx in sc["boxes"]])))
        return dict(wall=wall, icp=float(tm.stage_ms[3]), total=float(tm.stage_ms[4]), pairs=(tm.icp_pair_tests_hi << 32) | (tm.icp_pair_tests_lo & 0xffffffff), true=true_slot)
    modes = ("off", "fit", "select")
    for m in modes:
        call(m)
    runs = {m: [] for m in modes}
    for _ in range(reps):
        for m in modes:
            runs[m].append(call(m))
    print("the same call, %d interleaved calls each (host-fed cd_process_batch, %d frames):" % (reps, n_scenes))
    print("| setting | stage [3] ms median / min / max | device ms median / min / max | wall ms median / min / max | ICP pair tests | clusters reporting their true slot |")
    print("|---|---|---|---|---|---|")
    fmt = lambda v: "%.3f / %.3f / %.3f" % (float(np.median(v)), min(v), max(v))
    for m in modes:
        print("| %s | %s | %s | %s | %.3g | %d of %d |" % ({"off": "nothing set (all pairs)", "fit": "box fit", "select": "box fit + selection"}[m], fmt([r["icp"] for r in runs[m]]),
                                                       fmt([r["total"] for r in runs[m]]), fmt([r["wall"] for r in runs[m]]), runs[m][-1]["pairs"], runs[m][-1]["true"], len(picks)))
    print()
    ctx.close()


def worst_leg(reps):
    from perception_amd import capi
    i = np.arange(1024, dtype=np.int64)
    para = np.stack([i, i * i], 1)
    rng = np.random.RandomState(1)
    ctx = capi.Context(max_points=4096, max_frames=1)
    co = np.array([0, 0, 1, 0], np.float32)
    print("GPU, worst leg: one set per cd_box_fit_points call, a 1024-vertex hull (u = i, v = i^2) and points inside it; wall ms of the call, median of %d" % reps)
    print("| points | hull vertices | wall ms median / min / max |")
    print("|---|---|---|")
    for extra in (0, 5000, 50000):
        a = rng.randint(1, 1023, extra)
        inner = np.stack([a, a * a + 1 + (rng.randint(0, 1 << 30, extra) % np.maximum(1023 * a - a * a - 1, 1))], 1)     # (above the parabola, below its chord)
        uv = np.r_[para, inner]
        xyz = ((np.c_[uv, np.full(len(uv), 2000)].astype(np.float64) + 0.5) / 65536.0).astype(np.float32)
        ctx.box_fit_points([co], [xyz])
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = ctx.box_fit_points([co], [xyz])[0]
            t.append((time.perf_counter() - t0) * 1e3)
        print("| %d | %d (status %d) | %.3f / %.3f / %.3f |" % (len(xyz), r["hull_vertices"], r["status"], float(np.median(t)), min(t), max(t)))
    print()
    ctx.close()


def cost_leg(n_frames, reps):
    from perception_amd import capi, templates
    frames = frames_of(n_frames)
    prm = capi.default_params()
    prm.rgb_offset = 12
    ctx = capi.Context(max_points=frames.shape[1], max_frames=n_frames)
    ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))

    def call(on):
        ctx.set_box_fit(on)
        t0 = time.perf_counter()
        ctx.process_batch(frames, prm)
        wall = (time.perf_counter() - t0) * 1e3
        tm = ctx.timing()
        out = dict(wall=wall, icp=float(tm.stage_ms[3]), total=float(tm.stage_ms[4]), clusters=0, points=0)
        if on:
            res = [c for f in range(n_frames) for c in ctx.cluster_results(f)]
            out.update(clusters=len(res), points=sum(c.size for c in res))
        return out
    for on in (False, True):
        call(on)                                 # warm-up of each
    runs = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):                 # alternately: the settings share whatever else the machine is doing
            runs[on].append(call(on))
    last = runs[True][-1]
    print("GPU, cost leg: %d bench frames, %d interleaved calls each (host-fed cd_process_batch): %d clusters, %d points" % (n_frames, reps, last["clusters"], last["points"]))
    print("| step | stage [3] ms (stage_ms[3]) median / min / max | device ms (stage_ms[4]) median / min / max | wall ms median / min / max |")
    print("|---|---|---|---|")
    fmt = lambda v: "%.3f / %.3f / %.3f" % (float(np.median(v)), min(v), max(v))
    for on in (False, True):
        print("| %s | %s | %s | %s |" % ("on" if on else "off", fmt([r["icp"] for r in runs[on]]), fmt([r["total"] for r in runs[on]]), fmt([r["wall"] for r in runs[on]])))
    med = lambda on, key: float(np.median([r[key] for r in runs[on]]))
    print("the step costs %.3f ms of stage [3] (on minus off, medians), %.3f ms of the device total, %.3f ms of wall time\n"
          % (med(True, "icp") - med(False, "icp"), med(True, "total") - med(False, "total"), med(True, "wall") - med(False, "wall")))
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synth-frames", type=int, default=48)
    ap.add_argument("--config5-scenes", type=int, default=8)
    ap.add_argument("--cost-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--leg", choices=("synth", "config5", "cost", "worst"), default=None, help="run one leg in this process")
    args = ap.parse_args()
    if args.leg == "synth":
        synth_leg(args.synth_frames)
        return 0
    if args.leg == "config5":
        config5_leg(args.config5_scenes, args.reps)
        return 0
    if args.leg == "cost":
        cost_leg(args.cost_frames, args.reps)
        return 0
    if args.leg == "worst":
        worst_leg(args.reps)
        return 0
    # each leg in a fresh child process under its own time limit; a leg that fails, faults or runs out of time ends the report
    for leg in ("synth", "config5", "cost", "worst"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--synth-frames", str(args.synth_frames), "--config5-scenes", str(args.config5_scenes),
               "--cost-frames", str(args.cost_frames), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("the %s leg ran out of its %d s: nothing further is started" % (leg, args.limit))
            return 124
        if r.returncode != 0:
            print("the %s leg ended with status %d: nothing further is started" % (leg, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
