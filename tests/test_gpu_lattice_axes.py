"""The mask-free face code of k_icp_lat for templates with at most one face per constant axis (lat_nearest_axes,
perception_amd/csrc/k_icp_lat.hip; IcpLattice::axes_distinct) - through the C-ABI, against the same yardsticks as the general
face loop (tests/test_gpu_lattice.py):
 * cd_template_nearest against a numpy brute force with the oracle's arithmetic ((dx*dx + dy*dy) + dz*dz in float32, lowest
   original index on ties) for small lattices with every face order, two faces, one face, and two faces on ONE axis (which
   must keep the general code).  cd_template_nearest evaluates the one-face-per-axis form whenever the template qualifies and
   reports NaN for d2 where it disagrees with the general form in distance, neighbour or index;
 * the ICP on a permuted-face-order and a two-face template through launch shapes of k_icp_lat: records byte-identical to the
   generic search (CUBOID_ICP_LATTICE=0) and equal to the oracle;
 * one launch that mixes a one-face-per-axis template with the six-face one."""
import functools
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from perception_amd import capi, pcd, synth, templates

F32 = np.float32
# exact in float32, steps 1/4, 1/2, 1/8; each constant one step below its table, so that lattice nodes lie on bisecting planes
TABS = {0: np.arange(-1.0, 1.01, 0.25), 1: np.arange(-1.0, 1.01, 0.5), 2: np.arange(0.0, 0.51, 0.125)}   # 9 / 5 / 5 entries
CONST = {0: -1.25, 1: -1.5, 2: -0.125}


def _lattice(faces):
    """faces: [(constant axis, fast axis, constant)] -> (M, 3) float32, each face first-axis-fastest, faces one after the other."""
    out = []
    for w, u, c in faces:
        v = 3 - w - u
        uu, vv = np.meshgrid(TABS[u], TABS[v])
        p = np.empty((uu.size, 3))
        p[:, u] = uu.ravel(); p[:, v] = vv.ravel(); p[:, w] = c
        out.append(p)
    return np.concatenate(out, 0).astype(F32), np.repeat(np.arange(len(faces)), [len(p) for p in out])


def _face(w, fast_low=True):
    others = [a for a in range(3) if a != w]
    return (w, others[0] if fast_low else others[1], CONST[w])


CASES = [("order %d%d%d" % o, [_face(w, fast_low=(k != 1)) for k, w in enumerate(o)], 1) for o in itertools.permutations(range(3))]
CASES += [("two faces z x", [_face(2), _face(0, False)], 1), ("two faces y z", [_face(1), _face(2)], 1), ("one face y", [_face(1)], 1),
          ("two faces on z and one on x", [(2, 0, -0.125), (0, 1, -1.25), (2, 1, 0.625)], 0)]


def _queries(P):
    """~4096 queries: random near and far, lattice nodes (some lie on the bisecting plane of two faces), cell midpoints along one
    and along two axes (in-face ties), +-300 and +-30 000 along a face normal (float32 ties across a whole face), non-finite coordinates."""
    rng = np.random.default_rng(11)
    node = np.stack([g.ravel() for g in np.meshgrid(TABS[0], TABS[1], TABS[2], indexing="ij")], 1)   # 225 nodes of the axis tables
    half = np.array([0.125, 0.25, 0.0625])
    Q = [rng.uniform(-1.6, 1.6, (1200, 3)), rng.uniform(-40, 40, (300, 3)), node]
    for a in range(3):
        e = np.zeros(3); e[a] = half[a]
        Q.append(node + e)                                   # midway between two entries along one axis
        Q.append(node + half - e)                            # ... along the two other axes
    far = P[rng.integers(len(P), size=600)].astype(np.float64)
    far[np.arange(600), rng.integers(3, size=600)] += rng.choice([-300.0, 300.0, -30000.0, 30000.0], 600)   # (30 km: every in-plane term is below the rounding of the sum)
    Q.append(far)
    Q.append(P[rng.integers(len(P), size=200)].astype(np.float64) + rng.normal(0, 1e-4, (200, 3)))
    bad = rng.uniform(-1, 1, (24, 3))
    bad[np.arange(24), np.arange(24) % 3] = np.tile([np.nan, np.inf, -np.inf, np.nan], 6)
    Q.append(bad)
    return np.concatenate(Q, 0).astype(F32)


def _brute(P, face_of, Q):
    """Oracle arithmetic, first minimum.  Returns (index, d2, faces at the minimum, points of the winning face at the minimum)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (Q[:, None, 0] - P[None, :, 0]).astype(F32); dy = (Q[:, None, 1] - P[None, :, 1]).astype(F32); dz = (Q[:, None, 2] - P[None, :, 2]).astype(F32)
        d = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
        d = (d + (dz * dz).astype(F32)).astype(F32)
    idx = np.argmin(d, 1).astype(np.int32)                   # (first minimum; a row of NaN: 0)
    d2 = d[np.arange(len(Q)), idx]
    at_min = d == d2[:, None]
    nfaces = np.array([len(set(face_of[m])) for m in at_min])
    in_face = np.array([int((m & (face_of == face_of[i])).sum()) for m, i in zip(at_min, idx)])
    return idx, d2, nfaces, in_face


@functools.lru_cache(maxsize=None)
def _case(k):
    name, faces, distinct = CASES[k]
    P, face_of = _lattice(faces)
    Q = _queries(P)
    return name, P, Q, distinct, _brute(P, face_of, Q)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_the_queries_hold_the_tie_cases(k):
    """No GPU: the inputs of the test below really contain what they are meant to force."""
    name, P, Q, distinct, (idx, d2, nfaces, in_face) = _case(k)
    assert 3500 <= len(Q) <= 4500 and 25 <= len(P) <= 900
    finite = np.isfinite(Q).all(1)
    assert (in_face[finite] >= 2).sum() >= 1, name                                  # an in-face tie: the walk
    assert (in_face[finite] >= 9).sum() >= 1, name                                  # ... across a good part of a face
    if len(CASES[k][1]) >= 2:
        assert (nfaces[finite] >= 2).sum() >= 1, name                               # two faces at the same minimal d2: the face-order rule
    assert np.isnan(Q).any(1).sum() >= 6 and np.isinf(Q).any(1).sum() >= 6
    assert capi.lattice_axes(P)[0] == distinct, name


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)))
def test_nearest_equals_brute_force(k):
    name, P, Q, distinct, (bi, bd, _, _) = _case(k)
    ctx = capi.Context(max_points=8192, max_frames=1)
    try:
        ctx.set_template(0, P)
        assert ctx.template_lattice_faces(0) == len(CASES[k][1]), name
        idx, d2 = ctx.template_nearest(0, Q)
    finally:
        ctx.close()
    assert not np.isnan(d2).any(), name                       # (NaN = the one-face-per-axis form and the general form disagree)
    nanq = np.isnan(Q).any(1)
    # a query with a NaN coordinate compares below nothing: d2 = +inf as in the general face loop, any valid index
    assert np.all(d2[nanq] == np.inf) and np.all((idx[nanq] >= 0) & (idx[nanq] < len(P))), name
    ok = ~nanq                                                # (+-inf coordinates included: every d2 is +inf, index 0)
    assert np.array_equal(d2[ok].view(np.uint32), bd[ok].view(np.uint32)), name
    bad = np.nonzero(ok & (idx != bi))[0]
    assert len(bad) == 0, (name, Q[bad[:3]], idx[bad[:3]], bi[bad[:3]])


def _cuboid_faces(order, dims=(0.2, 0.1, 0.03, 0.002)):
    """The three faces make_cuboid_template writes (z = -H/2, y = -W/2, x = -L/2 as faces 0, 1, 2), in another order / a subset."""
    full = templates.template_xyz32(*dims)
    L, W, H, d = dims
    nx, ny, nz = len(np.arange(-L / 2, L / 2, d)), len(np.arange(-W / 2, W / 2, d)), len(np.arange(-H / 2, H / 2, d))
    cuts = np.cumsum([0, nx * ny, nx * nz, ny * nz])
    assert cuts[-1] == len(full)
    return np.concatenate([full[cuts[f]:cuts[f + 1]] for f in order], 0)


def _records_equal(a, b, where, accepted=True):
    assert (a.size, a.iterations, a.converged) == (b.size, b.iterations, b.converged), where
    assert not accepted or a.accepted == b.accepted, where
    assert list(a.T) == list(b.T) and a.fitness == b.fitness, where


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["", "1,1", "4,2", "8,1"])
@pytest.mark.parametrize("which", ["faces 2 0 1", "faces 0 1"])
def test_icp_through_the_launch_shapes(O, which, shape, monkeypatch):
    """Two frames through the fused call with a permuted-face-order template (x face, z face, y face) and a two-face template:
    records byte-identical to the generic search's, cluster results equal to the oracle's."""
    tpl = _cuboid_faces((2, 0, 1) if which == "faces 2 0 1" else (0, 1))
    assert capi.lattice_axes(tpl)[0] == 1
    if shape:
        monkeypatch.setenv("CUBOID_LAT_SHAPE", shape)
    frames = np.stack([synth.frame(i) for i in (100, 107)], 0)
    prm = capi.default_params()
    rec = {}
    for lattice in ("1", "0"):
        monkeypatch.setenv("CUBOID_ICP_LATTICE", lattice)
        ctx = capi.Context(max_points=frames.shape[1], max_frames=len(frames))
        try:
            ctx.set_template(0, tpl)
            res, _, _ = ctx.process_batch(frames, prm)
            assert ctx.timing().icp_search == (1 if lattice == "1" else 0)
            rec[lattice] = capi.results_to_array(res).copy()
            if lattice == "1":
                for f in range(len(frames)):
                    ro = O.process_frame(frames[f], prm, tpl)["result"]
                    assert res[f].n_clusters == ro.n_clusters and ro.n_clusters >= 1
                    for k in range(min(ro.n_clusters, capi.CD_MAX_CLUSTERS_PER_FRAME)):
                        _records_equal(res[f].clusters[k], ro.clusters[k], (f, k))
        finally:
            ctx.close()
    assert np.array_equal(rec["1"], rec["0"])


@pytest.mark.gpu
def test_one_launch_mixes_both_face_forms(template, monkeypatch):
    """template_slot = -1 with a one-face-per-axis template in slot 0 and the six-face template in slot 1: slots of one workgroup
    hold clusters of either kind.  Every cluster's record equals the better of the two single-template runs, and the whole batch
    the generic search's."""
    big = (pcd.read_xyz(os.path.join(GOLDEN, "template_cuboid_L200_W100_H75.pcd")).astype(F32) - F32([0.1, 0.05, 0.0375])).astype(F32)
    assert capi.lattice_axes(template)[0] == 1 and capi.lattice_axes(big)[0] == 0 and len(capi.lattice_detect(big)) == 6
    monkeypatch.setenv("CUBOID_LAT_SHAPE", "4,2,3")           # slots are refilled: a slot changes template
    frames = np.stack([synth.frame(i) for i in (30, 31)], 0)
    prm = capi.default_params()
    runs = {}
    for lattice in ("1", "0"):
        monkeypatch.setenv("CUBOID_ICP_LATTICE", lattice)
        ctx = capi.Context(max_points=frames.shape[1], max_frames=len(frames))
        try:
            ctx.set_template(0, template)
            ctx.set_template(1, big)
            for slot in ((-1,) if lattice == "0" else (-1, 0, 1)):
                prm.template_slot = slot
                res, _, _ = ctx.process_batch(frames, prm)
                if lattice == "1":
                    assert ctx.timing().icp_search == 1
                runs[(lattice, slot)] = (capi.results_to_array(res).copy(), [ctx.cluster_results(f) for f in range(len(frames))])
        finally:
            ctx.close()
    assert np.array_equal(runs[("1", -1)][0], runs[("0", -1)][0])
    seen = set()
    for f in range(len(frames)):
        mixed, per = runs[("1", -1)][1][f], [runs[("1", s)][1][f] for s in (0, 1)]
        assert len(mixed) == len(per[0]) == len(per[1]) >= 1
        for s in (0, 1):                                      # the single-template runs really used their own template
            assert all(c.template_slot == s for c in per[s]), (f, s)
        assert any(list(a.T) != list(b.T) for a, b in zip(per[0], per[1])), f
        for k, c in enumerate(mixed):
            assert c.template_slot in (0, 1)
            _records_equal(c, per[c.template_slot][k], (f, k), accepted=False)
            seen.add(c.template_slot)
    assert seen   # (which template wins is the data's business; both were searched for every cluster)
