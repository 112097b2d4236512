"""The plane stage on the device (S2: k_ransac_sample, k_ransac_count, k_plane_cov; the flags of S3: k_plane_flag_count,
k_extract_scatter) held to the float64 truth of tests/plane_reference.py on the committed case set of tests/plane_cases.py - the
assertions and tolerances tests/test_plane_truth_cpu.py holds the CPU oracle to - stand-alone and inside the fused batch call,
in batches whose frames stop in different hypothesis rounds, and at the sampler's three exits: PCL's own "no sample could be
selected", and the two limits of the device (the table of RND_TABLE random draws, the fill limit of the large shuffle map), where
the library must say CD_ERR_CAPACITY instead of returning the best model so far."""
import numpy as np
import pytest

import plane_cases as CS
import plane_reference as REF
from perception_amd import capi

pytestmark = pytest.mark.gpu

ROWS = 6208                        # rows of a frame of the fused tests: the largest case and some padding
MAX_POINTS = 8192
PAD = np.float32([0.0, 0.0, 2.0])  # outside the default crop
RND_TABLE, MAP_FILL = 1 << 15, 6144   # the device's limits (common.hpp: RND_TABLE, 3/4 SAMPLER_MAP)


@pytest.fixture(scope="module")
def ctx(template):
    cx = capi.Context(max_points=MAX_POINTS, max_frames=len(CS.truth_set()))
    cx.set_template(0, template)
    yield cx
    cx.close()


def frame_of(P, rows=ROWS):
    """the cloud as a frame: its points in REVERSE order (the voxel stage has to put them back), then padding outside the crop"""
    f = np.tile(PAD, (rows, 1))
    f[:len(P)] = P[::-1]
    return f


def record_fields(r):
    return (r.status, r.n_cropped, r.n_voxels, r.n_plane, r.n_objects, r.n_clusters, r.ransac_iterations)


# ---- 1. stand-alone ------------------------------------------------------------------------------------------------------------

def test_segment_plane_meets_the_truth(ctx, O):
    """cd_segment_plane on every case under every parameter set: iteration count, model and inlier indices against the truth.
    The unrefined model (plane_optimize = 0) is also the oracle's bit for bit: it is the sampler's own arithmetic, which a refit
    hides everywhere else."""
    runs = 0
    for name, n, rnd, P, tr in CS.truth_set():
        for t in CS.PARAMS:
            st, coeff, inl, it = ctx.segment_plane(P, CS.params(t))
            REF.assert_against_truth(tr[t], st, coeff, inl, it, t[0], "cd_segment_plane %s %s" % (name, t))
            if not t[0]:
                so, co, io, ito = O.segment_plane(P, CS.params(t))
                assert (st, it) == (so, ito) and coeff.tobytes() == co.tobytes() and np.array_equal(inl, io), (name, t, coeff, co)
            runs += 1
    assert runs == 34 * 24


# ---- 2. fused ------------------------------------------------------------------------------------------------------------------

def test_fused_batch_meets_the_truth(ctx, O):
    """Every case as a frame of cd_process_batch.  The cloud the plane stage sees is the oracle's voxel cloud of the frame, which is
    what the device reports and - one point per voxel, in voxel order - the case's points themselves."""
    cases = CS.truth_set()
    frames = np.stack([frame_of(P) for _, _, _, P, _ in cases])
    base = capi.default_params()
    for f, (name, n, _, P, _) in enumerate(cases):
        st, vox, _, nc, _ = O.crop_voxel(frames[f], base)
        assert st == 0 and nc == n and vox.tobytes() == P.tobytes(), name
    for t in CS.PARAMS:
        res, pi, _ = ctx.process_batch(frames, CS.params(t), want_indices=True)
        for f, (name, n, _, P, tr) in enumerate(cases):
            if t == CS.DEFAULTS:
                got = ctx.frame_cloud(f, capi.CD_CLOUD_VOXELS, 16, -1)[:, :3].copy().view(np.float32)
                assert got.tobytes() == P.tobytes(), name
            r = res[f]
            assert r.n_voxels == n and r.n_cropped == n, name
            assert r.status in (capi.CD_OK, capi.CD_ERR_NO_MODEL), (name, r.status)
            REF.assert_against_truth(tr[t], r.status, np.float32(list(r.plane)), pi[f][:r.n_plane], r.ransac_iterations, t[0],
                                     "cd_process_batch %s %s" % (name, t))
            assert (pi[f][r.n_plane:] == -1).all(), name


# ---- 3. frames that finish in different rounds ---------------------------------------------------------------------------------

def collinear_cloud():
    """3000 points on x = y = z at steps of 2^-13: isSampleGood rejects every sample"""
    return np.outer(np.arange(1, 3001) / 8192.0, [1.0, 1.0, 1.0]).astype(np.float32)


def test_batches_of_frames_that_stop_in_different_rounds(ctx, O, template):
    """One batch with a frame for each round of 16, 64, 256 and 1040 hypotheses, a frame of two voxels, an empty frame and a frame
    whose every sample is rejected, in two orders: each frame's record and indices are, byte for byte, those of the frame alone in
    a batch of one, they are the oracle's, and the case frames meet the truth."""
    cases = {name: (P, tr) for name, _, _, P, tr in CS.truth_set()}
    names = ["n2049_round1", "n2048_round2", "n2047_round3", "n6145_round4", "n65_round3", "n4097_round2"]
    two = np.tile(PAD, (ROWS, 1))
    two[:2] = [[0.01, 0.02, 0.3], [-0.05, 0.1, 0.5]]
    pool = [(nm, frame_of(cases[nm][0])) for nm in names]
    pool += [("two voxels", two), ("empty", np.tile(PAD, (ROWS, 1))), ("collinear", frame_of(collinear_cloud()))]
    prm = capi.default_params()
    iters = [cases[nm][1][CS.DEFAULTS]["iterations"] for nm in names[:4]]
    assert iters[0] <= 16 < iters[1] <= 64 < iters[2] <= 256 < iters[3], iters
    alone, oracle = {}, {}
    for nm, fr in pool:
        res, pi, lb = ctx.process_batch(fr[None], prm, want_indices=True)
        alone[nm] = (capi.results_to_array(res).tobytes(), pi[0].tobytes(), lb[0].tobytes())
        oracle[nm] = O.process_frame(fr, prm, template)
    for order in (list(range(len(pool))), [3, 8, 0, 6, 2, 7, 5, 1, 4]):
        res, pi, lb = ctx.process_batch(np.stack([pool[k][1] for k in order]), prm, want_indices=True)
        rec = capi.results_to_array(res)
        for f, k in enumerate(order):
            nm = pool[k][0]
            r, o = res[f], oracle[nm]
            assert (rec[f:f + 1].tobytes(), pi[f].tobytes(), lb[f].tobytes()) == alone[nm], (nm, order)
            assert record_fields(r) == record_fields(o["result"]), (nm, record_fields(r), record_fields(o["result"]))
            assert bytes(r.plane) == bytes(o["result"].plane) and np.array_equal(pi[f][:r.n_plane], o["plane_inliers"]), nm
            if nm in cases:
                REF.assert_against_truth(cases[nm][1][CS.DEFAULTS], r.status, np.float32(list(r.plane)), pi[f][:r.n_plane],
                                         r.ransac_iterations, 1, "mixed batch %s" % nm)
        by_name = {pool[k][0]: res[f] for f, k in enumerate(order)}
        assert record_fields(by_name["two voxels"])[:3] == (capi.CD_ERR_NO_MODEL, 2, 2)
        assert by_name["empty"].n_voxels == 0 and by_name["empty"].ransac_iterations == 0
        assert by_name["collinear"].status == capi.CD_ERR_NO_MODEL and by_name["collinear"].ransac_iterations == 0


# ---- 4. the sampler's exits ----------------------------------------------------------------------------------------------------

def test_no_sample_could_be_selected(ctx, O):
    """PCL's own stop, 1000 rejected samples in a row: CD_ERR_NO_MODEL after 0 iterations, as the oracle has it.  (As a frame of a
    batch: test_batches_of_frames_that_stop_in_different_rounds.)"""
    P = collinear_cloud()
    assert sampler_limit(P, 1) == ("no sample", 0)
    so, _, io, ito = O.segment_plane(P, capi.default_params())
    assert (so, len(io), ito) == (capi.CD_ERR_NO_MODEL, 0, 0)
    st, _, inl, it = ctx.segment_plane(P, capi.default_params())
    assert (st, len(inl), it) == (capi.CD_ERR_NO_MODEL, 0, 0)


def sampler_limit(P, hypotheses):
    """The device's sampler replayed on the host (the reference's shuffle, the float32 ratio test of isSampleGood): which exit it
    takes within `hypotheses` hypotheses and at which one - "table": a draw would read past RND_TABLE numbers; "map": the shuffle
    map has no room for a draw's 6 slots; "no sample": PCL's 1000 checks - or (None, hypotheses)."""
    s = REF.Sampler(len(P), draws=RND_TABLE + 3)
    for h in range(hypotheses):
        good = False
        for _ in range(REF.MAX_SAMPLE_CHECKS):
            if s.rp + 3 > RND_TABLE:
                return "table", h
            if len(s.map) + 6 > MAP_FILL:
                return "map", h
            i0, i1, i2 = s.draw()
            with np.errstate(all="ignore"):
                q = (P[i1] - P[i0]) / (P[i2] - P[i0])
            if q[0] != q[1] or q[2] != q[1]:
                good = True
                break
        if not good:
            return "no sample", h
    return None, hypotheses


def line_cloud(n, on_line, grid):
    """on_line of n points on the line x = y = z - 0.5 at multiples of 2^-2 / grid (every sample of three of them is rejected),
    the rest scattered"""
    rng = np.random.RandomState(41)
    t = rng.permutation(grid)[:on_line].astype(np.float64) / grid * 0.25
    pts = np.concatenate([np.stack([t, t, t + 0.5], 1), rng.uniform(-0.1, 0.1, (n - on_line, 3)) + [0, 0, 0.5]])
    return pts[rng.permutation(n)].astype(np.float32)


def no_inlier_params(max_iterations):
    """a threshold no point passes: PCL's loop runs to plane_max_iterations + 1"""
    prm = capi.default_params()
    prm.plane_distance_threshold = 0.0
    prm.plane_max_iterations = max_iterations
    return prm


@pytest.mark.parametrize("n, on_line, grid, limit, at", [(3000, 2970, 4096, "table", 308), (8000, 7760, 8192, "map", 308)],
                         ids=["random table", "shuffle map"])
def test_a_device_limit_of_the_sampler_is_reported(ctx, O, n, on_line, grid, limit, at):
    """99 % (97 %) of the cloud on a line of exactly representable points: some 35 (11) rejected samples per hypothesis, so the
    device's sampler runs out of random numbers (of room in its shuffle map) at hypothesis `at`, which the host's replay shows.
    The oracle, like PCL, has no such limit and runs to 1001 iterations.  The library must not pass off its best model so far:
    CD_ERR_CAPACITY, with the limits in cd_last_error - and the oracle's answer, bit for bit, as long as PCL's loop ends within
    the hypotheses the device could draw."""
    P = line_cloud(n, on_line, grid)
    assert sampler_limit(P, 1001) == (limit, at)
    assert O.segment_plane(P, no_inlier_params(1000))[3] == 1001
    for max_iter in (at, 1000):                          # hypothesis `at` (counting from 0) is the first one missing
        with pytest.raises(capi.CuboidError) as e:
            ctx.segment_plane(P, no_inlier_params(max_iter))
        assert e.value.status == capi.CD_ERR_CAPACITY and "hypothesis %d" % at in str(e.value) and "%d random draws" % RND_TABLE in str(e.value)
    for max_iter in (at - 1, 5):
        prm = no_inlier_params(max_iter)
        so, co, io, ito = O.segment_plane(P, prm)
        st, coeff, inl, it = ctx.segment_plane(P, prm)
        assert (st, it) == (so, ito) == (capi.CD_OK, max_iter + 1) and coeff.tobytes() == co.tobytes() and np.array_equal(inl, io)


def voxel_line_cloud():
    """102 points on the line (t, 4 t, 4 t), t at multiples of 2^-9 - one per 5 mm voxel of the default crop, in voxel order - and two
    points off it: 17 draws per hypothesis, the table of random draws is used up at hypothesis 639"""
    t = np.arange(1, 103) / 512.0
    pts = np.concatenate([np.stack([t, 4 * t, 4 * t], 1), [[0.1, 0.0, 0.3], [-0.1, 0.2, 0.6]]]).astype(np.float32)
    cell = np.floor(pts.astype(np.float64) / CS.LEAF).astype(np.int64)
    return pts[np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))]


def test_a_device_limit_inside_a_batch_fails_that_frame_alone(ctx, O, template):
    """In a batch the frame's status carries CD_ERR_CAPACITY, the call returns CD_OK and the frames beside it are what they are
    without it; with plane_max_iterations below the limit the frame is the oracle's again."""
    P = voxel_line_cloud()
    assert sampler_limit(P, 1001) == ("table", 639)
    cases = {name: (q, tr) for name, _, _, q, tr in CS.truth_set()}
    a, b = "n2049_round1", "n2047_round3"
    frames = np.stack([frame_of(cases[a][0]), frame_of(P), frame_of(cases[b][0])])
    for max_iter, fails in ((1000, True), (639, True), (638, False)):
        prm = no_inlier_params(max_iter)
        res, pi, _ = ctx.process_batch(frames, prm, want_indices=True)
        if max_iter == 1000:
            got = ctx.frame_cloud(1, capi.CD_CLOUD_VOXELS, 16, -1)[:, :3].copy().view(np.float32)
            assert got.tobytes() == P.tobytes()
        for f in (0, 1, 2):
            o = O.process_frame(frames[f], prm, template)["result"]
            if f == 1 and fails:
                assert o.status == capi.CD_OK and o.ransac_iterations == max_iter + 1      # (PCL: the first model, without an inlier)
                assert res[f].status == capi.CD_ERR_CAPACITY and res[f].n_plane == 0 and res[f].n_voxels == len(P)
                assert tuple(res[f].plane) == (0.0, 0.0, 0.0, 0.0) and (pi[f] == -1).all()
            else:
                assert record_fields(res[f]) == record_fields(o) and bytes(res[f].plane) == bytes(o.plane), (f, max_iter)
