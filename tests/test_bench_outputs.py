"""bench.py --dump-outputs: the records the timed path returned in its last step, one float32 / float64 .npy per field, so
that two builds can be compared output for output.  On the device: a plain run (no --full) prints the contract's fields,
leaves the post-timing checks to --full, and its dump equals a serial pass over the same frames, field by field."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["cluster_T", "cluster_pose", "cluster_stats", "frame_counts", "plane"]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_record_field(tmp_path):
    import bench
    from perception_amd import capi
    rec = (capi.CdFrameResult * 3)()
    rec[1].n_voxels, rec[1].n_clusters, rec[2].status = 1234, 2, capi.CD_ERR_NO_MODEL
    rec[2].plane[3] = -0.75
    rec[1].clusters[1].size, rec[1].clusters[1].iterations, rec[1].clusters[1].fitness = 300, 41, 2.5e-4
    rec[1].clusters[1].T[3] = 0.125
    rec[1].clusters[0].pose[7] = -1.0 / 3.0
    bench.dump_outputs(capi.results_to_array(rec), str(tmp_path / "all"))
    got = _load(tmp_path / "all")
    assert sorted(got) == FIELDS
    assert all(a.dtype in (np.float32, np.float64) and a.shape[0] == 3 for a in got.values())
    assert got["frame_counts"].shape == (3, 8) and got["frame_counts"][1, 2] == 1234 and got["frame_counts"][1, 5] == 2
    assert got["frame_counts"][2, 0] == capi.CD_ERR_NO_MODEL
    assert got["plane"][2, 3] == np.float32(-0.75)
    assert got["cluster_stats"].shape == (3, capi.CD_MAX_CLUSTERS_PER_FRAME, 6)
    assert list(got["cluster_stats"][1, 1]) == [300, 41, 0, 0, 0, 2.5e-4]
    assert got["cluster_T"][1, 1, 3] == np.float32(0.125)
    assert got["cluster_pose"][1, 0, 7] == -1.0 / 3.0
    # above the cap: a fixed sample, the same every time, with its frame numbers
    old = bench.DUMP_MAX_FRAMES
    try:
        bench.DUMP_MAX_FRAMES = 2
        bench.dump_outputs(capi.results_to_array(rec), str(tmp_path / "a"))
        bench.dump_outputs(capi.results_to_array(rec), str(tmp_path / "b"))
    finally:
        bench.DUMP_MAX_FRAMES = old
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(FIELDS + ["frame_index"]) and len(a["frame_index"]) == 2
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["frame_index"].astype(int)
    assert np.array_equal(a["frame_counts"], got["frame_counts"][rows])


@pytest.mark.gpu
def test_plain_run_dumps_the_records_of_its_last_step(tmp_path):
    import bench
    from perception_amd import capi, templates
    F = 16
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(F), "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "bench")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["metric"]
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["verified"] is None and out["single_frame_ms"] is None and out["config5"] is None and "cpu_baseline" not in out
    got = _load(tmp_path / "bench")
    assert sorted(got) == FIELDS and sum(a.nbytes for a in got.values()) <= 64 << 20
    frames = bench.make_frames(0, F)
    prm = capi.default_params()
    prm.rgb_offset = 12
    ctx = capi.Context(max_points=frames.shape[1], max_frames=F)
    try:
        ctx.set_template(0, templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
        rec = capi.results_to_array(ctx.process_batch(frames, prm)[0]).copy()
    finally:
        ctx.close()
    bench.dump_outputs(rec, str(tmp_path / "serial"))
    want = _load(tmp_path / "serial")
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["frame_counts"][:, 5].sum() > 0          # the batch has clusters: the comparison covers ICP results
