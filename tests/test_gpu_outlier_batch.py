"""The outlier filter (rule C16) as a step of the fused calls, checked by composition: a call with the filter off gives every
frame's object cloud; the numpy module (perception_amd/outlier_filter.py) filters it; a call with the filter on must then hold
exactly that cloud - xyz and colour, byte for byte - and everything behind it must be what the oracle's clustering and ICP give
on that cloud.  The switch leaves nothing behind, the depth-fed call does the same, and the point labels (rule C15) follow the
filtered call's own outputs."""
import struct

import numpy as np
import pytest

from perception_amd import capi, outlier_filter as OF, point_labels as PL, synth

pytestmark = pytest.mark.gpu
MEAN_K, STD_MUL = 16, 1.0


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _snapshot(ctx, res, pi, lb):
    """Everything a fused call returns and leaves to be read, as plain arrays."""
    F = len(res)
    return dict(res=capi.results_to_array(res).copy(), pi=pi.copy(), lb=lb.copy(),
                obj=[ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, 12).copy() for f in range(F)],
                vox=[ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12).copy() for f in range(F)],
                clusters=[[np.frombuffer(c, np.uint8).copy() for c in ctx.cluster_results(f)] for f in range(F)])


def _same_snapshot(a, b):
    assert np.array_equal(a["res"], b["res"]) and np.array_equal(a["pi"], b["pi"]) and np.array_equal(a["lb"], b["lb"])
    for key in ("obj", "vox"):
        assert len(a[key]) == len(b[key]) and all(np.array_equal(x, y) for x, y in zip(a[key], b[key]))
    assert all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a["clusters"], b["clusters"]))


def _check_filtered_call(ctx, O, template, prm, off, res, lb):
    """Call B against the module's filter of call A's object clouds and the oracle's stages behind it.  Returns (points removed
    per frame, frames that passed untouched)."""
    removed, untouched = [], 0
    for f in range(len(res)):
        want, o = OF.filter_cloud(off["obj"][f], MEAN_K, STD_MUL)
        got = ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, 12)
        r = res[f]
        st = ctx.outlier_stats(f)
        print("frame %d: n_o %d -> %d (module %d), computed %d, clusters %d" % (f, len(off["obj"][f]), r.n_objects, len(want), o["computed"], r.n_clusters))
        assert got.shape == want.shape and np.array_equal(got, want), "frame %d: the filtered object cloud differs" % f
        assert r.n_objects == len(want)
        assert (st["n_before"], st["n_removed"]) == (len(off["obj"][f]), len(off["obj"][f]) - len(want))
        assert [_bits(st[k]) for k in ("mean", "stddev", "threshold")] == [_bits(o[k]) for k in ("mean", "stddev", "threshold")]
        removed.append(st["n_removed"])
        untouched += st["n_removed"] == 0
        xyz = np.ascontiguousarray(want[:, :3]).view(np.float32)
        l0, s0, k0 = O.cluster(xyz, prm, mode=1, sizes_capacity=64)
        assert r.n_clusters == k0 and np.array_equal(lb[f][:r.n_objects], l0) and (lb[f][r.n_objects:] == -1).all()
        recs = ctx.cluster_results(f)
        assert [c.size for c in recs] == list(s0[:k0])
        for k in range(min(k0, capi.CD_MAX_CLUSTERS_PER_FRAME)):
            pts = xyz[l0 == k]
            s, r0, _ = O.icp(template, pts, prm, nn_mode=1)
            c = r.clusters[k]
            assert s == 0 and list(c.T) == list(r0.T), "frame %d cluster %d: T" % (f, k)
            assert (c.fitness, c.iterations, c.converged, c.size) == (r0.fitness, r0.iterations, r0.converged, len(pts))
            assert np.array_equal(ctx.cluster_points(f, k)[:, :3].view(np.uint32), pts.view(np.uint32))
    return removed, untouched


@pytest.fixture(scope="module")
def batch(frames4):
    """frames4, frame 0 with flying pixels, and a frame without a box (an empty object cloud) in the context's last slot."""
    fly = synth.flying_pixels(frames4[0], synth.WIDTH, synth.HEIGHT, seed=7, frac=0.5)
    return np.ascontiguousarray(np.stack(list(frames4) + [fly, synth.frame(4, k_obj=0)], 0))


@pytest.fixture(scope="module")
def ctx(template, batch):
    c = capi.Context(max_points=batch.shape[1], max_frames=batch.shape[0])
    c.set_template(0, template)
    yield c
    c.close()


@pytest.fixture(scope="module")
def calls(ctx, batch):
    """Call A (off), call B (on) with its labels, call A again (off): the GPU work every test below reads."""
    prm = capi.default_params()
    prm.rgb_offset = 12
    assert ctx.outlier_filter_setting()[0] == 0
    off = _snapshot(ctx, *ctx.process_batch(batch, prm, want_indices=True))
    labels_off = ctx.label_points_last(batch)
    with pytest.raises(capi.CuboidError):
        ctx.outlier_stats(0)                       # that call ran without the filter
    ctx.set_outlier_filter(MEAN_K, STD_MUL, False)
    res, pi, lb = ctx.process_batch(batch, prm, want_indices=True)
    on = dict(res=res, pi=pi, lb=lb)
    return dict(prm=prm, off=off, labels_off=labels_off, on=on)


def test_fused_call_equals_the_module_and_the_oracle_behind_it(ctx, O, template, batch, calls):
    prm, off, on = calls["prm"], calls["off"], calls["on"]
    ctx.set_outlier_filter(MEAN_K, STD_MUL, False)
    res, pi, lb = ctx.process_batch(batch, prm, want_indices=True)      # (idempotent: the fixture's call B again)
    assert np.array_equal(capi.results_to_array(res), capi.results_to_array(on["res"])) and np.array_equal(lb, on["lb"])
    removed, untouched = _check_filtered_call(ctx, O, template, prm, off, res, lb)
    assert max(removed) > 0 and untouched >= 1, "the batch shows nothing: no frame lost points, or none passed untouched"
    assert removed[5] == 0 and res[5].n_objects == 0                   # the context's last slot is the degenerate frame
    assert removed[4] != removed[0]                                     # the flying pixels changed what the filter saw
    assert np.array_equal(pi, off["pi"])                                # the plane is upstream of the filter
    for f in range(len(res)):
        assert np.array_equal(ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, 12), off["vox"][f])
    # the labels of the filtered call from its own outputs; a removed voxel's points read GATED
    got = ctx.label_points_last(batch)
    for f in range(len(res)):
        r = res[f]
        vox = off["vox"][f][:, :3].copy().view(np.float32)
        obj = ctx.frame_cloud(f, capi.CD_CLOUD_OBJECTS, 16, -1)[:, :3].copy().view(np.float32)
        want = PL.labels_of_frame(batch[f], prm, r.n_voxels, pi[f][:r.n_plane], vox, obj, lb[f][:r.n_objects])
        assert np.array_equal(got[f], want), "frame %d: %d labels differ" % (f, int((got[f] != want).sum()))
    gated = (got == capi.CD_LABEL_GATED) & (calls["labels_off"] != capi.CD_LABEL_GATED)
    print("input points that the filter turned to CD_LABEL_GATED:", int(gated.sum()))
    assert gated.any() and not ((got != capi.CD_LABEL_GATED) & (calls["labels_off"] == capi.CD_LABEL_GATED)).any()
    # another compute call invalidates the statistics with the other read-backs
    ctx.outlier_filter(np.zeros((4, 3), np.float32), 2)
    with pytest.raises(capi.CuboidError):
        ctx.outlier_stats(0)


def test_switching_the_filter_off_leaves_nothing_behind(ctx, batch, calls):
    ctx.set_outlier_filter(0)
    again = _snapshot(ctx, *ctx.process_batch(batch, calls["prm"], want_indices=True))
    _same_snapshot(again, calls["off"])
    assert np.array_equal(ctx.label_points_last(batch), calls["labels_off"])
    with pytest.raises(capi.CuboidError):
        ctx.outlier_stats(0)


def test_depth_fed_call(ctx, O, template):
    cam = capi.default_depth_camera()
    cam.fx, cam.fy, cam.cx, cam.cy = synth.depth_camera_params()
    cam.depth_scale = synth.DEPTH_SCALE
    cam.color = capi.CD_COLOR_RGB8
    pairs = [synth.depth_frame(i) for i in (0, 2)]
    depth = np.ascontiguousarray(np.stack([p[0] for p in pairs]))
    color = np.ascontiguousarray(np.stack([p[1] for p in pairs]))
    prm = capi.default_params()
    ctx.set_outlier_filter(0)
    off = _snapshot(ctx, *ctx.process_depth_batch(depth, color, cam, prm, want_indices=True))
    ctx.set_outlier_filter(MEAN_K, STD_MUL, False)
    res, pi, lb = ctx.process_depth_batch(depth, color, cam, prm, want_indices=True)
    removed, _ = _check_filtered_call(ctx, O, template, prm, off, res, lb)
    assert min(removed) > 0
    assert all(c[:, 3].any() for c in off["obj"])                      # the colour travels with the point
    ctx.set_outlier_filter(0)
    _same_snapshot(_snapshot(ctx, *ctx.process_depth_batch(depth, color, cam, prm, want_indices=True)), off)


def test_process_frame_and_negative(ctx, frames4):
    """cd_process_frame takes the setting too; negative keeps exactly what the positive filter removes."""
    prm = capi.default_params()
    prm.rgb_offset = 12
    ctx.set_outlier_filter(0)
    ctx.process_frame(frames4[1], prm)
    base = ctx.frame_cloud(0, capi.CD_CLOUD_OBJECTS, 16, 12).copy()
    for negative in (False, True):
        ctx.set_outlier_filter(50, 0.5, negative)
        r, _, _ = ctx.process_frame(frames4[1], prm)
        want, o = OF.filter_cloud(base, 50, 0.5, negative)
        assert r.n_objects == len(want) and np.array_equal(ctx.frame_cloud(0, capi.CD_CLOUD_OBJECTS, 16, 12), want)
        assert 0 < len(want) < len(base)
    ctx.set_outlier_filter(0)
