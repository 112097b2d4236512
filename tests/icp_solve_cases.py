"""The case set of the ICP solve's truth tests (tests/test_icp_solve_truth_cpu.py, tests/test_gpu_icp_solve_truth.py): one
deterministic generator of about 2 500 records (16 fixed-point moment sums of rule C4, n, an incoming ICP_STATE), used by the CPU
and the GPU test alike.  Sums are built as tests/test_gpu_icp_solve_row.py builds them (sums_from) from sigma = U diag(s) V^T with
random rotations; a record's class is DECIDED by the float64 SVD of the sigma recomputed from its integer sums, not by the
generator's numbers (quantisation to 2^-32 moves small singular values): a draw that misses its class is drawn again.

    A  400  full rank, det > 0: S0 in 1e-6 .. 1, S1/S0 and S2/S0 in 0.05 .. 1 (a quarter: near-identity motions, which meet the
            epsilon and MSE exits of the convergence tail)
    B  400  det < 0: |S2|/S0 in 0.05 .. 1; a quarter with S1 - |S2| down to 1e-3 S0
    C  400  exact rank 2, s = (s0, +-s1, 0), S1/S0 in 0.05 .. 1, zero means and n = 1: the sums hold sigma itself
    D  400  rank 2 by the 1e-5 threshold: recomputed |S2|/S0 < 3e-6, either sign, S0 in 1e-3 .. 1, S1/S0 in 0.05 .. 1
    E  200  moments of real pairs summed term by term (rule C4): q = 3 .. 300 points of ONE face of the default lattice template
            (exactly planar), p = q moved by up to 5 degrees and 1 cm plus 0.5 mm of noise, the scene shifted by up to 1 m
    F  200  the rank threshold straddled: |S2|/S0 in 0.5e-5 .. 2e-5, S1/S0 in 0.3 .. 1
    G  500  degenerate: zero, rank 1 (dense and sparse), S1 = S2 with det < 0, the twenty STRUCTURED matrices at n = 1, 3, 1000

NaN-producing inputs (n = 0, sums at the ends of their range) are not here: they stay in the row-equals-lane tests."""
import functools

import numpy as np

from perception_amd import capi, templates
from test_gpu_icp_solve_row import M64, STRUCTURED, rot, sums_from

CRITERIA = [("default", dict()), ("eps", dict(trans_eps=1e-3)), ("abs", dict(abs_mse=1e-5)), ("rel", dict(rel_mse=0.5)),
            ("limit", dict(max_iter=3))]            # the five sets of test_gpu_icp_solve_row.py
CLASS_SIZES = dict(A=400, B=400, C=400, D=400, E=200, F=200, G=500)


def sigma_of(sums, n):
    """float64 sigma = E[q p^T] - mq mp^T of one record's integer sums (as icp_solve_reference.moments, for one record)."""
    s = np.array([(int(v) ^ (1 << 63)) - (1 << 63) for v in sums[:15]], np.float64) * 2.0 ** -32 / float(n)
    return s[6:15].reshape(3, 3) - np.outer(s[3:6], s[0:3])


def _signed_sv(sg):
    """(S0, S1, d * S2) of a float64 sigma: the third singular value carries the sign of det U det V."""
    U, S, Vt = np.linalg.svd(sg)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    return S[0], S[1], d * S[2]


def _loguni(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _draw(rng, make, accept):
    """make() -> (sums, n) until accept(S0, S1, signed S2) holds for the recomputed sigma."""
    for _ in range(200):
        sums, n = make()
        if accept(*_signed_sv(sigma_of(sums, n))):
            return sums, n
    raise AssertionError("a class of the case set cannot be drawn")


def _from_s(rng, s, n=None, means=True, identity=False, mse=None):
    U = rot(rng)
    V = U if identity else rot(rng)
    sg = (U @ np.diag(s) @ V.T).ravel()
    n = int(rng.integers(3, 2000)) if n is None else n
    mp = rng.uniform(-1, 1, 3) if means else np.zeros(3)
    mq = (mp + rng.uniform(-1e-5, 1e-5, 3) * int(rng.integers(0, 3)) if identity else rng.uniform(-1, 1, 3)) if means else np.zeros(3)
    return sums_from(n, mp, mq, sg, rng.uniform(0, 1e-3) if mse is None else mse), n


def _faces(tpl):
    """The three faces of the default lattice template in the order templates.make_cuboid_template writes them: z = -H/2
    (100 x 50 points), y = -W/2 (100 x 15), x = -L/2 (50 x 15); each exactly planar along its axis."""
    assert len(tpl) == 7250
    faces = [tpl[:5000], tpl[5000:6500], tpl[6500:]]
    assert all(len(np.unique(f[:, a])) == 1 for f, a in zip(faces, (2, 1, 0)))
    return faces


def _real_pairs(rng, faces):
    from conftest import rot_xyz
    face = faces[int(rng.integers(3))]
    k = int(rng.integers(3, 301))
    shift = rng.uniform(-1, 1, 3)
    q0 = face[rng.choice(len(face), size=k, replace=False)].astype(np.float64)
    p0 = q0 @ rot_xyz(*np.deg2rad(rng.uniform(-5, 5, 3))).T + rng.uniform(-0.01, 0.01, 3) + rng.normal(0, 0.0005, q0.shape)
    q, p = (q0 + shift).astype(np.float32), (p0 + shift).astype(np.float32)
    assert any(len(np.unique(q[:, a])) == 1 for a in range(3))           # still exactly planar after the shift
    d2 = ((q[:, 0] - p[:, 0]) ** 2 + (q[:, 1] - p[:, 1]) ** 2) + (q[:, 2] - p[:, 2]) ** 2
    terms = [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [q[:, a] * p[:, b] for a in range(3) for b in range(3)]
    s = [int(np.rint(t.astype(np.float64) * 2.0 ** 32).astype(np.int64).sum()) & M64 for t in terms]
    s.append(int(np.rint(d2.astype(np.float64) * 2.0 ** 36).astype(np.int64).sum()) & M64)
    return s, k


@functools.lru_cache(maxsize=None)
def case_set():
    """dict(sums uint64 [K, 16], n int32 [K], states ICP_STATE [K], cls '<U1' [K], mse float64 [K]); treat it as read-only."""
    rng = np.random.default_rng(20240521)
    sums, ns, cls = [], [], []

    def add(c, rec):
        sums.append(rec[0]); ns.append(rec[1]); cls.append(c)

    for i in range(CLASS_SIZES["A"]):
        def make():
            s0 = _loguni(rng, 1e-6, 1)
            s1 = s0 * rng.uniform(0.05, 1)
            return _from_s(rng, [s0, s1, s1 * rng.uniform(0.05 * s0 / s1, 1)], identity=(i % 4 == 3), mse=1e-4 if i % 4 == 3 else None)
        add("A", _draw(rng, make, lambda S0, S1, S2: 1e-6 <= S0 <= 1.01 and S1 >= 0.05 * S0 and S2 >= 0.05 * S0))
    for i in range(CLASS_SIZES["B"]):
        def make():
            s0 = _loguni(rng, 1e-3, 1)
            if i % 4 == 3:
                s1 = s0 * rng.uniform(0.06, 1)
                s2 = max(s1 - s0 * _loguni(rng, 1.05e-3, 0.5), 0.05 * s0)
            else:
                s1 = s0 * rng.uniform(0.05, 1)
                s2 = s1 * rng.uniform(0.05 * s0 / s1, 1)
            return _from_s(rng, [s0, s1, -s2])
        add("B", _draw(rng, make, lambda S0, S1, S2: S2 < 0 and -S2 >= 0.05 * S0 and S1 + S2 >= 1e-3 * S0))
    for i in range(CLASS_SIZES["C"]):
        def make():
            s0 = rng.uniform(0.1, 1)
            return _from_s(rng, [s0, s0 * rng.uniform(0.05, 1) * (1 if i % 2 else -1), 0.0], n=1, means=False)
        add("C", _draw(rng, make, lambda S0, S1, S2: S1 >= 0.05 * S0 and abs(S2) < 1e-8 * S0))
    for i in range(CLASS_SIZES["D"]):
        def make():
            s0 = _loguni(rng, 1e-3, 1)
            return _from_s(rng, [s0, s0 * rng.uniform(0.05, 1), s0 * rng.uniform(-2.5e-6, 2.5e-6)])
        want = 1 if i % 2 else -1          # either sign, as recomputed
        add("D", _draw(rng, make, lambda S0, S1, S2: 1e-3 <= S0 <= 1.01 and S1 >= 0.05 * S0 and abs(S2) < 3e-6 * S0 and S2 * want > 0))
    faces = _faces(templates.template_xyz32(**templates.DEFAULT_TEMPLATE))
    assert [len(f) for f in faces] == [5000, 1500, 750]
    for i in range(CLASS_SIZES["E"]):
        add("E", _real_pairs(rng, faces))
    for i in range(CLASS_SIZES["F"]):
        def make():
            s0 = _loguni(rng, 1e-2, 1)
            return _from_s(rng, [s0, s0 * rng.uniform(0.3, 1), s0 * _loguni(rng, 0.5e-5, 2e-5) * (1 if i % 2 else -1)])
        add("F", _draw(rng, make, lambda S0, S1, S2: S1 >= 0.3 * S0 and 0.5e-5 * S0 <= abs(S2) <= 2e-5 * S0))
    for sg in STRUCTURED:
        for n in (1, 3, 1000):
            add("G", (sums_from(n, np.zeros(3), np.zeros(3), sg, 1e-4), n))
    for i in range(40):                                                  # zero covariance, with and without means
        n = (1, 3, 7, 1000)[i % 4]
        m = rng.uniform(-1, 1, 3) * min(i // 4, 1)
        add("G", (sums_from(n, m, m, np.zeros(9), 1e-4), n))
    for i in range(250):                                                 # rank 1: dense (150), sparse (100: one entry, zero means)
        if i < 150:
            add("G", _from_s(rng, [rng.uniform(0.01, 1), 0.0, 0.0], n=1, means=False))
        else:
            sg = np.zeros(9)
            sg[int(rng.integers(9))] = rng.uniform(0.01, 1) * rng.choice([-1, 1])
            n = int(rng.integers(3, 2000))
            add("G", (sums_from(n, np.zeros(3), np.zeros(3), sg, 1e-4), n))
    for i in range(150):                                                 # S1 = S2 with det < 0: R* is a one-parameter family
        s0 = rng.uniform(0.1, 1)
        s1 = s0 * rng.uniform(0.05, 1)
        add("G", _from_s(rng, [s0, s1, -s1]))
    K = len(ns)
    assert K == sum(CLASS_SIZES.values()) and all(cls.count(c) == k for c, k in CLASS_SIZES.items())
    sums = np.array(sums, np.uint64)
    ns = np.array(ns, np.int32)
    mse = np.array([((int(v) ^ (1 << 63)) - (1 << 63)) * 2.0 ** -36 for v in sums[:, 15]]) / ns
    st = np.zeros(K, capi.ICP_STATE)                                    # incoming states as in test_gpu_icp_solve_row.py
    for i in range(K):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rot(rng), rng.uniform(-1, 1, 3)
        st["Tfinal"][i] = T.astype(np.float32).ravel()
    st["T"] = rng.uniform(-1, 1, (K, 16)).astype(np.float32)
    st["prev_mse"] = np.where(rng.integers(0, 4, K) == 0, np.finfo(np.float64).max, rng.uniform(0, 1e-3, K))
    st["prev_mse"][3::8] = mse[3::8] * (1 + 1e-9)      # an MSE that repeats: the absolute test; ... [7::8] one nearby: the relative one
    st["prev_mse"][7::8] = mse[7::8] * (1 + 1e-7)
    st["iters"] = rng.integers(0, 6, K)
    st["status"] = 7
    out = dict(sums=sums, n=ns, states=st, cls=np.array(cls), mse=mse)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- single-face clusters end to end (tests/test_gpu_icp_planar_known_answer.py and its CPU twin) ----
PLANAR_SEEDS = (0, 1, 2)


def planar_scenes(tpl):
    """Nine scenes: the interior points of one face of the default template - 300 of the large face, all of the two thin ones,
    the outermost row of the face left out on every side - moved by a rotation of up to 0.1 degrees per axis and a translation
    of up to 0.3 mm per axis, three seeds each.  dict(face, seed, origin (template indices), src float32 [n, 3], motion float64
    4 x 4: src = motion . tpl[origin], rounded to float32)."""
    from conftest import rot_xyz
    out = []
    for f, (lo, hi, axis) in enumerate(((0, 5000, 2), (5000, 6500, 1), (6500, 7250, 0))):
        pts = tpl[lo:hi].astype(np.float64)
        inner = np.ones(hi - lo, bool)
        for a in range(3):
            if a != axis:
                inner &= (pts[:, a] > pts[:, a].min() + 1e-3) & (pts[:, a] < pts[:, a].max() - 1e-3)
        inner = lo + np.flatnonzero(inner)
        assert len(inner) == ((98 * 48, 98 * 13, 48 * 13)[f])
        for seed in PLANAR_SEEDS:
            rng = np.random.default_rng(1000 * f + seed)
            origin = np.sort(rng.choice(inner, size=300, replace=False)) if f == 0 else inner
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = rot_xyz(*np.deg2rad(rng.uniform(-0.1, 0.1, 3))), rng.uniform(-0.0003, 0.0003, 3)
            src = (tpl[origin].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
            out.append(dict(face=f, seed=seed, origin=origin, src=src, motion=M))
    return out


def planar_table_params():
    """The launch values, with the crops opened below z = 0 (the template sits at the origin) and a 1 mm leaf: lattice points are
    2 mm apart, so every point is the only one of its voxel and its centroid is the point itself."""
    prm = capi.default_params()
    prm.crop_z_min = prm.crop2_z_min = -0.5
    prm.leaf_size = 0.001
    return prm


def planar_table_frames(scenes):
    """One frame per scene, float32 [F, N, 3]: the scene's moved face above a synthetic table (the plane z = 0.1, 4 mm pitch,
    4 186 points - more than any face, 87 mm and more from it), padded with NaN records to one length.  The fused call finds the
    table, removes it and is left with the face as its only cluster."""
    tx, ty = np.meshgrid(np.arange(-0.18, 0.1801, 0.004), np.arange(-0.09, 0.0901, 0.004))
    table = np.stack([tx.ravel(), ty.ravel(), np.full(tx.size, 0.1)], axis=1).astype(np.float32)
    n = len(table) + max(len(s["src"]) for s in scenes)
    frames = np.full((len(scenes), n, 3), np.nan, np.float32)
    for f, s in enumerate(scenes):
        frames[f, :len(table)] = table
        frames[f, len(table):len(table) + len(s["src"])] = s["src"]
    return frames


def same_point_set(a, b):
    """Two float32 [n, 3] arrays hold the same points, in any order."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a[np.lexsort(a.T)].view(np.uint32), b[np.lexsort(b.T)].view(np.uint32))
