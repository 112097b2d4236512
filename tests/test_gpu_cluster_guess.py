"""Rule C13 on the GPU: cd_shape_frames (k_shape.hip) against the plain-Python restatement byte for byte, and CD_GUESS_CLUSTER
through the fused call and cd_icp against the oracle's ICP started from the restated guess - T bits, iterations, fitness and
accepted of every cluster, under every ICP driver."""
import numpy as np
import pytest

from perception_amd import capi, cluster_frame as cf, pcd, synth
from conftest import GOLDEN

import os

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (3, 63, 64, 65, 255, 256, 257, 1400, 25000)   # around the wave (64) and the workgroup (256); several strided rounds


def point_sets():
    rng = np.random.default_rng(77)
    out = []
    for i, n in enumerate(SIZES):
        R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        p = rng.standard_normal((n, 3)) * rng.uniform(0.01, 0.4, 3)
        centre = rng.uniform(0.2, 1.0, 3) * np.array([1.0, -1.0, 1.0]) * (1.0 if i % 2 else 20.0)   # far from the origin too: large sums
        out.append((p @ R.T + centre).astype(F32))
    assert all((s < 0).any() and (s > 0).any() and np.abs(s).max() < 64 for s in out)   # coordinates of both signs, inside C4's range
    return out


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(max_points=4096, max_frames=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def restated_sets():
    sets = point_sets()
    return sets, [cf.shape_frame(s).to_bytes() for s in sets]


@pytest.mark.parametrize("stride", [12, 16, 32])
def test_shape_frames_equal_restatement(ctx, restated_sets, stride):
    sets, want = restated_sets
    cols = stride // 4
    wide = []
    for s in sets:
        w = np.full((s.shape[0], cols), np.nan, F32)   # whatever follows x, y, z in a record is not read
        w[:, :3] = s
        wide.append(w)
    got = ctx.shape_frames(wide)
    for i, s in enumerate(sets):
        assert got[i].n == s.shape[0] and got[i].status == capi.CD_OK
        assert bytes(got[i]) == want[i], "set %d (n = %d), stride %d" % (i, s.shape[0], stride)
        assert bytes(capi.shape_frame_host(s)) == want[i]


def test_refused_set_among_good_ones(ctx, restated_sets):
    sets, want = restated_sets
    for bad_value in (np.nan, 64.5):
        dirty = [s.copy() for s in sets]
        dirty[4][200, 1] = bad_value                   # set 4 (255 points), a lane of the last wave
        got = ctx.shape_frames(dirty)
        for i in range(len(sets)):
            if i == 4:
                assert got[i].status == capi.CD_ERR_INVALID_ARG and bytes(got[i]) == cf.shape_frame(dirty[4]).to_bytes()
            else:
                assert bytes(got[i]) == want[i]
    tiny = [sets[0][:2], np.zeros((0, 3), F32), sets[1]]  # too small sets are results as well
    got = ctx.shape_frames(tiny)
    assert [g.status for g in got] == [capi.CD_ERR_FEW_CORRESPONDENCES, capi.CD_ERR_FEW_CORRESPONDENCES, capi.CD_OK]
    assert all(bytes(g) == cf.shape_frame(t).to_bytes() for g, t in zip(got, tiny))


# ---- the fused call ------------------------------------------------------------------------------------------------------------

def same_cluster(a, b):
    assert (a.size, a.iterations, a.converged, a.accepted, a.template_slot) == (b["size"], b["iterations"], b["converged"], b["accepted"], b["slot"])
    assert list(a.T) == b["T"], "final transformation not bit-identical"
    assert a.fitness == b["fitness"]


@pytest.fixture(scope="module")
def scene(O, template):
    """Two 640 x 480 frames (one box, three boxes), their oracle clusters, the restated records and, against each of two templates,
    the oracle's ICP of every cluster started from the restated guess (CD_GUESS_PARAMS): computed once, shared, unchanged."""
    tpl2 = pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75_3faces.pcd")).astype(F32)
    tpls = [template, tpl2]
    trec = [cf.shape_frame(t) for t in tpls]
    frames = [synth.frame(0, k_obj=1), synth.frame(1, k_obj=3)]
    prm = capi.default_params()
    clusters, recs, per, plain = [], [], [], []
    for f in frames:
        o = O.process_frame(f, prm, template, want_clouds=True)
        K = o["result"].n_clusters
        srcs = [o["objects"][o["labels"] == k] for k in range(K)]
        clusters.append(srcs)
        recs.append([cf.shape_frame(s) for s in srcs])
        plain.append(o["result"])
        per_cluster = []
        for s, r in zip(srcs, recs[-1]):
            per_tpl = []
            for t in (0, 1):
                G, flip = cf.guess(r, trec[t])
                assert flip >= 0
                p = capi.default_params()
                p.icp_use_guess = capi.CD_GUESS_PARAMS
                p.icp_guess[:] = [float(v) for v in G.ravel()]
                st, res, _ = O.icp(tpls[t], s, p)
                assert st == 0
                per_tpl.append(dict(size=res.size, iterations=res.iterations, converged=res.converged, accepted=res.accepted,
                                    T=list(res.T), fitness=res.fitness))
            per_cluster.append(per_tpl)
        per.append(per_cluster)
    assert [len(c) for c in clusters] == [1, 3]
    return dict(frames=np.stack(frames, 0), tpls=tpls, trec=trec, clusters=clusters, recs=recs, per=per, plain=plain)


def wanted(scene, f, order):
    """Frame f's clusters when slot s holds template order[s]: the lower fitness is kept, ties keep the lowest slot."""
    out = []
    for per_tpl in scene["per"][f]:
        best = None
        for slot, t in enumerate(order):
            if best is None or per_tpl[t]["fitness"] < best["fitness"]:
                best = dict(per_tpl[t], slot=slot)
        out.append(best)
    return out


def run_mode(scene, order):
    c = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=2)
    try:
        for s, t in enumerate(order):
            c.set_template(s, scene["tpls"][t])
            assert bytes(c.template_shape_frame(s)) == scene["trec"][t].to_bytes()
        prm = capi.default_params()
        prm.icp_use_guess = capi.CD_GUESS_CLUSTER
        prm.template_slot = 0 if len(order) == 1 else -1
        res, _, _ = c.process_batch(scene["frames"], prm)
        for f in range(2):
            want = wanted(scene, f, order)
            assert res[f].status == capi.CD_OK and res[f].n_clusters == len(want)
            assert res[f].flags & capi.CD_FRAME_CLUSTER_GUESS
            for k, w in enumerate(want):
                same_cluster(res[f].clusters[k], w)
            got = c.cluster_shape_frames(f)
            assert [bytes(g) for g in got] == [r.to_bytes() for r in scene["recs"][f]]
        assert bytes(c.cluster_shape_frames(1, first=1, count=1)[0]) == scene["recs"][1][1].to_bytes()
    finally:
        c.close()


@pytest.mark.parametrize("env", [{}, {"CUBOID_ICP_MODE": "sliced"}, {"CUBOID_ICP_MODE": "cluster"}, {"CUBOID_ICP_MODE": "pipe"},
                                 {"CUBOID_ICP_LATTICE": "0"}, {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_PERSIST": "0"},
                                 {"CUBOID_ICP_LATTICE": "0", "CUBOID_ICP_PERSIST": "2"}],   # (2: the persistent launch hands over to the multi-launch loop)
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()) or "auto")
def test_fused_call_equals_oracle_from_restated_guess(scene, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_mode(scene, [0])


def test_fused_call_two_template_slots(scene):
    """Slot 0 holds the 75 mm template, slot 1 the default one (which wins): every pair's guess comes from its slot's record."""
    assert all(w["slot"] == 1 for f in range(2) for w in wanted(scene, f, [1, 0]))
    run_mode(scene, [1, 0])


def test_mode_leaves_no_state_behind(scene):
    c = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=2)
    try:
        c.set_template(0, scene["tpls"][0])
        plain, guessed = capi.default_params(), capi.default_params()
        guessed.icp_use_guess = capi.CD_GUESS_CLUSTER
        before = bytes(capi.results_to_array(c.process_batch(scene["frames"], plain)[0]))
        with pytest.raises(capi.CuboidError):               # the records exist after a call in the mode only
            c.cluster_shape_frames(0)
        mid = c.process_batch(scene["frames"], guessed)[0]
        assert len(c.cluster_shape_frames(1)) == 3
        after = bytes(capi.results_to_array(c.process_batch(scene["frames"], plain)[0]))
        assert before == after
        assert bytes(capi.results_to_array(mid)) != before
        with pytest.raises(capi.CuboidError) as e:
            c.cluster_shape_frames(0)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
        res = capi.results_from_array(np.frombuffer(after, np.uint8).reshape(2, -1))
        for f in range(2):                                  # the default path is the oracle's identity start, flag clear
            assert not (res[f].flags & capi.CD_FRAME_CLUSTER_GUESS)
            for k in range(res[f].n_clusters):
                assert list(res[f].clusters[k].T) == list(scene["plain"][f].clusters[k].T)
    finally:
        c.close()


@pytest.mark.parametrize("env", [{}, {"CUBOID_ICP_LATTICE": "0"}], ids=["lat", "generic"])
def test_cd_icp_in_the_mode(scene, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(max_points=synth.WIDTH * synth.HEIGHT, max_frames=2)
    try:
        c.set_template(0, scene["tpls"][0])
        prm = capi.default_params()
        prm.icp_use_guess = capi.CD_GUESS_CLUSTER
        c.process_batch(scene["frames"], prm)
        assert len(c.cluster_shape_frames(0)) == 1
        for f in range(2):
            for k, src in enumerate(scene["clusters"][f]):
                st, r, _ = c.icp(0, src, prm)
                assert st == capi.CD_OK
                same_cluster(r, wanted(scene, f, [0])[k])
        with pytest.raises(capi.CuboidError) as e:          # cd_icp is not a fused call: its records are not kept
            c.cluster_shape_frames(0)
        assert e.value.status == capi.CD_ERR_INVALID_ARG
        st, r, _ = c.icp(0, scene["clusters"][0][0][:2], prm)   # too small a source: no frame, no guess, PCL's refusal as ever
        assert st == capi.CD_ERR_FEW_CORRESPONDENCES and list(r.T) == [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    finally:
        c.close()
