"""The lattice ICP's row solve (icp_step_row: a slot's step on a row of 16 lanes) end to end, at the smallest shapes where the
lane mapping can go wrong: one frame with 1, 3, 5 and 9 clusters of 93 .. 186 points against the default three-face template,
forced through the launch shapes
    1,1 (one row)   1,8 (the alone shape)   2,2   4,2 (the in-flight shape: a full solving wave)   8,1 / 8,2 (slots 4-7 on wave 1)
so that a row set is partly filled (1 and 3 clusters in 4 or 8 slots, 5 in 8), refills leave rows empty while others iterate
(9 clusters with 12 .. 77 iterations each in 2, 4 or 8 slots), and a finished slot's write-back runs beside solving rows of the
same wave.  Records == the CPU oracle == the generic-search drivers (CUBOID_ICP_LATTICE=0), byte for byte; once more with a
maximum correspondence distance that rejects nothing (10 m), which runs the BOUNDED kernels to the same records, and with one that
does reject (1 cm: the 4 cm boxes do not fit the template, so every step keeps a different subset) - there the oracle has no
say (it has no bound), and the records must equal the generic-search drivers', whose solve is the single-lane icp_step."""
import numpy as np
import pytest

from perception_amd import capi, synth

pytestmark = pytest.mark.gpu

GRIDS = {1: (1, 1), 3: (3, 1), 5: (5, 1), 9: (3, 3)}
SHAPES = ["1,1", "1,8", "2,2", "4,2", "8,1", "8,2"]
REJECTING = 0.01


def params():
    p = capi.default_params()
    p.cluster_min_size = 60
    return p


@pytest.fixture(scope="module")
def scenes(O, template):
    """{clusters: (frame, the oracle's records of every cluster)}, computed once."""
    out = {}
    for k, (cols, rows) in GRIDS.items():
        frame = synth.render(synth.scene_grid(3, cols=cols, rows=rows, dims=(0.04, 0.04, 0.03), jitter=0.7))
        o = O.process_frame(frame, params(), template, all_clusters=64)
        assert o["result"].n_clusters == k and len(o["clusters"]) == k
        assert all(70 <= c.size <= 200 for c in o["clusters"]), [c.size for c in o["clusters"]]
        out[k] = (frame, o["clusters"])
    assert len({c.iterations for c in out[9][1]}) >= 6      # the rows of a wave finish at different rounds
    return out


def records(monkeypatch, template, frame, env, dist=None):
    for key in ("CUBOID_LAT_SHAPE", "CUBOID_ICP_LATTICE"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    ctx = capi.Context(max_points=frame.shape[0], max_frames=1)
    try:
        ctx.set_template(0, template)
        if dist is not None:
            ctx.set_icp_max_correspondence_distance(dist)
        ctx.process_batch(frame[None], params())
        assert ctx.timing().icp_search == (0 if env.get("CUBOID_ICP_LATTICE") == "0" else 1)
        return ctx.cluster_results(0)
    finally:
        ctx.close()


def same(got, want, tag):
    assert len(got) == len(want), tag
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a.size, a.iterations, a.converged, a.accepted) == (b.size, b.iterations, b.converged, b.accepted), (tag, k)
        assert np.float32(list(a.T)).tobytes() == np.float32(list(b.T)).tobytes() and a.fitness == b.fitness, (tag, k)


@pytest.fixture(scope="module")
def generic(scenes, template):
    """The generic-search drivers' records of every scene (unbounded and bounded), computed once."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for k, (frame, _) in scenes.items():
            for dist in (None, 10.0, REJECTING):
                out[k, dist] = records(mp, template, frame, {"CUBOID_ICP_LATTICE": "0"}, dist)
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", list(GRIDS))
def test_row_solve_in_every_shape(monkeypatch, scenes, generic, template, k, shape):
    frame, want = scenes[k]
    got = records(monkeypatch, template, frame, {"CUBOID_LAT_SHAPE": shape})
    same(got, want, "oracle")
    same(got, generic[k, None], "generic")


@pytest.mark.parametrize("shape", SHAPES)
def test_row_solve_bounded(monkeypatch, scenes, generic, template, shape):
    for k in (3, 9):
        frame, want = scenes[k]
        got = records(monkeypatch, template, frame, {"CUBOID_LAT_SHAPE": shape}, dist=10.0)
        same(got, want, ("oracle", k))
        same(got, generic[k, 10.0], ("generic", k))


@pytest.mark.parametrize("shape", SHAPES)
def test_row_solve_with_a_bound_that_rejects(monkeypatch, scenes, generic, template, shape):
    """The kept-correspondence count of a slot (s_nv) is what the row divides by and takes the constants off with."""
    for k in (5, 9):
        frame, _ = scenes[k]
        want = generic[k, REJECTING]
        # the bound matters: these are not the unbounded records
        assert any(np.float32(list(a.T)).tobytes() != np.float32(list(b.T)).tobytes() or a.iterations != b.iterations
                   for a, b in zip(want, generic[k, None])), k
        same(records(monkeypatch, template, frame, {"CUBOID_LAT_SHAPE": shape}, dist=REJECTING), want, ("generic", k))
