"""icp_step_row (icp_solve_row.hpp: one ICP iteration's state update on a row of 16 lanes) against the single-lane icp_step on
the device, through cd_icp_solve_batch: both solvers of one launch, four records per wave.

The records are laid out so that the four rows of a wave differ: record 4g is a dense random covariance (several sweeps),
4g + 1 a structured one (zero, rank 1 / 2 with either sign of det U det V, det < 0, m00 + m11 == 0, y == 0 in make_jacobi,
diagonal: no rotation or a single one, the ends of the sums' range), 4g + 2 has fewer than three correspondences in every other
wave (the BOUNDED launch stops that row beside three running ones; the unbounded launch solves it, n = 0 giving inf and NaN
means), 4g + 3 is a near-identity motion that converges by another branch than its neighbours.  Row == single lane in every byte.
For moments the CPU oracle can express - the first iteration of an ICP of a small cluster - both equal the oracle's step.
The same entry compares sqrt_ge1 / rcp_ge1 with the IEEE operations for every float of their domain (3.2e9 evaluations).
The single-lane solver is the REFERENCE here; whether it is right is checked in tests/test_gpu_icp_solve_truth.py (and, on the
host, tests/test_icp_solve_truth_cpu.py) against a float64 Umeyama written from the definition."""
import numpy as np
import pytest

from conftest import rot_xyz
from perception_amd import capi, templates

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
STRUCTURED = [
    [0, 0, 0, 0, 0, 0, 0, 0, 0], [0.5, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0.25, 0, 0, 0, 0, 0, 0],
    [0.5, 0, 0, 0, 0.25, 0, 0, 0, 0], [0.5, 0, 0, 0, -0.25, 0, 0, 0, 0], [0, 0.5, 0, 0.25, 0, 0, 0, 0, 0],
    [0.5, 0, 0, 0, 0.25, 0, 0, 0, -0.125], [-0.5, 0, 0, 0, -0.25, 0, 0, 0, -0.125],
    [0.5, 0.25, 0, 0.125, -0.5, 0, 0, 0, 0.25], [0.5, 0.25, 0, -0.25, -0.5, 0, 0, 0, 0.25], [0.5, 0.25, 0, 0.25, -0.5, 0, 0, 0, 0.25],
    [0, 0.125, 0, 0, 0.5, 0, 0, 0, 0.25], [0.25, 0, 0, 0.125, 0, 0, 0, 0, 0.5],
    [0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5], [0.125, 0, 0, 0, 0.25, 0, 0, 0, 0.5], [0.25, 0, 0, 0, 0.5, 0, 0, 0, 0.125],
    [1, 1, 1, 1, 1, 1, 1, 1, 1], [1, 2, 3, 4, 5, 6, 7, 8, 9],
    [2147483647.0, 0, 0, 0, 2.0 ** -32, 0, 0, 0, 1], [2.0 ** -32, 2.0 ** -32, 0, 0, 2.0 ** -32, 0, 0, 0, 0],
]
ENDS = [0, 1, M64, 1 << 62, (-(1 << 62)) & M64, (1 << 63) - 1, 1 << 63]


def cluster_near(tpl, n, seed):
    """A source that starts near the template: a subset moved by a small rigid motion, plus 1 mm of noise."""
    rng = np.random.default_rng(seed)
    p = tpl[rng.choice(len(tpl), size=n, replace=False)].astype(np.float64)
    p = p @ rot_xyz(*np.deg2rad(rng.uniform(-3, 3, 3))).T + rng.uniform(-0.01, 0.01, 3) + rng.normal(0, 0.001, p.shape)
    return p.astype(np.float32)


def fix(v, shift):
    return int(np.rint(np.ldexp(np.float64(v), shift))) & M64


def sums_from(n, mp, mq, sg, mse):
    k = max(n, 1)
    out = [fix(k * mp[a], 32) for a in range(3)] + [fix(k * mq[a], 32) for a in range(3)]
    out += [fix(k * (sg[3 * a + b] + mq[a] * mp[b]), 32) for a in range(3) for b in range(3)]
    return out + [fix(k * mse, 36)]


def rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def batch():
    """(sums uint64 [K, 16], n int32 [K], states ICP_STATE [K]) - 4096 random records and the structured ones, interleaved."""
    rng = np.random.default_rng(20190409)
    sums, ns = [], []
    for g in range(1100):
        kind = g % 4
        sg = rng.uniform(-1, 1, 9)
        if kind == 1:
            sg *= 10.0 ** rng.uniform(-9, 3)
        if kind == 2:
            sg = (rot(rng) @ np.diag([rng.uniform(0.1, 1), rng.uniform(0.01, 0.1) * rng.choice([-1, 1]), 0.0]) @ rot(rng).T).ravel()
        mp, mq = (np.zeros(3), np.zeros(3)) if kind == 2 else (rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3))
        n = 1 if kind == 2 else int(rng.integers(3, 2000))
        sums.append(sums_from(n, mp, mq, sg, rng.uniform(0, 1e-3))); ns.append(n)                     # 4g: dense / scaled / rank 2
        if g < 10 * len(STRUCTURED):
            n = (1, 2, 3, 4, 1000, 3, 7, 50, 200, 1999)[g // len(STRUCTURED)]
            sums.append(sums_from(n, np.zeros(3), np.zeros(3), STRUCTURED[g % len(STRUCTURED)], 1e-4)); ns.append(n)
        else:
            sums.append([ENDS[i] if rng.integers(3) == 0 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2)) for i in rng.integers(0, 7, 16)])
            ns.append(int(rng.choice([1, 2, 3, 7, 2147483647, -1])))                                # 4g + 1: structured / extreme
        n = int(rng.integers(0, 3)) if g % 2 == 0 else int(rng.integers(3, 500))
        sums.append(sums_from(n, rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 9), 2e-4)); ns.append(n)   # 4g + 2: too few
        U = rot(rng)
        mp = rng.uniform(-1, 1, 3)
        sums.append(sums_from(500, mp, mp + rng.uniform(-1e-5, 1e-5, 3) * (g % 3), (U @ np.diag(rng.uniform(0.1, 1, 3)) @ U.T).ravel(), 1e-4))
        ns.append(500)                                                                                # 4g + 3: near identity
    K = len(ns)
    assert K == 4400
    st = np.zeros(K, capi.ICP_STATE)
    for i in range(K):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rot(rng), rng.uniform(-1, 1, 3)
        st["Tfinal"][i] = T.astype(np.float32).ravel()
    st["T"] = rng.uniform(-1, 1, (K, 16)).astype(np.float32)
    st["prev_mse"] = np.where(rng.integers(0, 4, K) == 0, np.finfo(np.float64).max, rng.uniform(0, 1e-3, K))
    st["prev_mse"][3::8] = 1e-4 * (1 + 1e-9)          # some near-identity rows meet the relative-MSE test
    st["iters"] = rng.integers(0, 6, K)
    st["status"] = 7
    return np.array(sums, np.uint64), np.array(ns, np.int32), st


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("crit", [dict(), dict(trans_eps=1e-3), dict(abs_mse=1e-5), dict(rel_mse=0.5), dict(max_iter=3)],
                         ids=["default", "eps", "abs", "rel", "limit"])
def test_row_equals_single_lane(batch, crit, bounded):
    sums, n, st = batch
    row, lane, done, _ = capi.icp_solve_batch(sums, n, st, bounded=bounded, **crit)
    diff = [i for i in range(len(n)) if row[i].tobytes() != lane[i].tobytes() or done[i, 0] != done[i, 1]]
    assert not diff, (len(diff), diff[:8], row[diff[0]], lane[diff[0]])
    few = n < 3
    if bounded:      # rule C8: the stopped rows - identity, nothing else moved - beside running ones in the same wave
        assert few[2::8].all() and (done[few, 0] == 1).all() and (row["converged"][few] == 0).all()
        assert (row["T"][few] == np.eye(4, dtype=np.float32).ravel()).all()
        assert (row["iters"][few] == st["iters"][few]).all() and row["Tfinal"][few].tobytes() == st["Tfinal"][few].tobytes()
    run = ~few if bounded else np.ones(len(n), bool)
    assert (row["iters"][run] == st["iters"][run] + 1).all()
    assert 0 < done[run, 0].sum() < run.sum()             # the rows of the launch end differently
    assert row["status"].tolist() == [7] * len(n) and not row["done"].any()


def test_row_equals_the_oracles_first_iteration(O):
    """What the oracle can express of a step: the first iteration of an ICP (Tfinal = identity going in), from the moments of
    the oracle's own correspondences summed by rule C4."""
    tpl = templates.template_xyz32(**templates.DEFAULT_TEMPLATE)
    prm = capi.default_params()
    prm.icp_max_iterations = 1
    sums, ns, want = [], [], []
    for seed, npts in enumerate((70, 93, 128, 200, 300, 64, 65, 199)):
        src = cluster_near(tpl, npts, 40 + seed)
        status, r, _ = O.icp(tpl, src, prm, nn_mode=1)
        assert status == 0 and r.iterations == 1
        idx, d2 = O.nn(tpl, src)
        p, q = src.astype(np.float32), tpl[idx].astype(np.float32)
        terms = [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [q[:, a] * p[:, b] for a in range(3) for b in range(3)]
        s = [int(np.rint(t.astype(np.float64) * 2.0 ** 32).astype(np.int64).sum()) & M64 for t in terms]
        s.append(int(np.rint(d2.astype(np.float64) * 2.0 ** 36).astype(np.int64).sum()) & M64)
        sums.append(s); ns.append(npts); want.append(np.float32(list(r.T)))
    st = np.zeros(len(ns), capi.ICP_STATE)
    st["Tfinal"] = np.eye(4, dtype=np.float32).ravel()
    st["prev_mse"] = np.finfo(np.float64).max
    row, lane, done, _ = capi.icp_solve_batch(np.array(sums, np.uint64), np.array(ns, np.int32), st, max_iter=1, trans_eps=prm.icp_transformation_epsilon,
                                              rel_mse=prm.icp_euclidean_fitness_epsilon)
    assert row.tobytes() == lane.tobytes() and done.tolist() == [[1, 1]] * len(ns)
    for i, w in enumerate(want):
        assert row["Tfinal"][i].tobytes() == w.tobytes() and row["T"][i].tobytes() == w.tobytes(), i


def test_short_forms_equal_ieee_for_every_float_of_their_domain():
    """sqrt_ge1 on [1, +inf] (1.07e9 floats) and rcp_ge1 on 1 <= |x| < 2^126 (2.1e9), the domains row_rotation keeps them to:
    no mismatch, or the library does not use the form."""
    sums, n, st = np.zeros((1, 16), np.uint64), np.array([5], np.int32), np.zeros(1, capi.ICP_STATE)
    un = capi.icp_solve_batch(sums, n, st, unary=True)[3]
    print("sqrt_ge1: %d mismatches (first input bits %#x), used %d; rcp_ge1: %d mismatches (first %#x), used %d" % (
        un[0], un[1], un[4], un[2], un[3], un[5]))
    assert un[0] == 0 or un[4] == 0
    assert un[2] == 0 or un[5] == 0
