"""Canonical rule C13 in plain Python: the principal frame of a point set and the rigid ICP guess that carries
a cluster's frame onto a template's.  numpy int64 for the fixed-point sums, Python floats (IEEE double, one operation at a
time) for everything else.  This restatement is the rule's DEFINITION: cd_shape_frame_host / cd_shape_guess equal it bit for bit
and the device (k_shape.hip: cd_shape_frames, CD_GUESS_CLUSTER) byte for byte.  CPU only; nothing here touches the GPU.
"""
import math

import numpy as np

CD_OK, CD_ERR_INVALID_ARG, CD_ERR_CAPACITY, CD_ERR_FEW_CORRESPONDENCES = 0, -1, -2, -5
COORD_MAX = 64.0          # rule C4's range
N_MAX = 1 << 19           # rule C4's count
SWEEPS = 8                # cyclic Jacobi sweeps, fixed
PAIRS = ((0, 1), (0, 2), (1, 2))
FLIPS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))
SIGMA_EPS = 2.0 ** -20


class ShapeFrame:
    """cd_shape_frame: n, status, mean[3], axes[9] (row-major, columns = axes), var[3], lo[3], hi[3]."""
    __slots__ = ("n", "status", "mean", "axes", "var", "lo", "hi")

    def __init__(self, n=0, status=CD_OK):
        self.n, self.status = int(n), int(status)
        self.mean, self.axes, self.var, self.lo, self.hi = [0.0] * 3, [0.0] * 9, [0.0] * 3, [0.0] * 3, [0.0] * 3

    def doubles(self):
        """The 21 doubles of the record in struct order."""
        return np.array(self.mean + self.axes + self.var + self.lo + self.hi, np.float64)

    def to_bytes(self):
        return np.array([self.n, self.status], np.int32).tobytes() + self.doubles().tobytes()


def moments(points):
    """Step 1a: the nine order-free sums (x, y, z, xx, xy, xz, yy, yz, zz) as Python ints."""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    terms = (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)   # float32 products: one IEEE multiply each
    # fixq(v, 32): float32 -> double (exact), times 2^32 (exact), round to nearest even -> int64; numpy's int64 sum wraps like the device's
    return [int(np.rint(t.astype(np.float64) * 4294967296.0).astype(np.int64).sum(dtype=np.int64)) for t in terms]


def jacobi(c):
    """Step 2 on the symmetric 3x3 c (list of rows): (eigenvalues[3], axes[9] row-major) sorted, right-handed."""
    a = [list(r) for r in c]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            apq = a[p][q]
            if apq == 0.0:
                continue
            r = 3 - p - q
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            root = math.sqrt(theta * theta + 1.0)
            t = 1.0 / (theta + root) if theta >= 0.0 else -1.0 / (root - theta)
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            h = t * apq
            a[p][p] = a[p][p] - h
            a[q][q] = a[q][q] + h
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = cs * arp - sn * arq
            a[r][q] = a[q][r] = sn * arp + cs * arq
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = cs * vkp - sn * vkq
                v[k][q] = sn * vkp + cs * vkq
    d = [a[0][0], a[1][1], a[2][2]]
    col = [[v[0][j], v[1][j], v[2][j]] for j in range(3)]
    for i, j in ((0, 1), (1, 2), (0, 1)):          # stable, descending: swap only when the later one is strictly larger
        if d[j] > d[i]:
            d[i], d[j] = d[j], d[i]
            col[i], col[j] = col[j], col[i]
    A = [col[0][0], col[1][0], col[2][0], col[0][1], col[1][1], col[2][1], col[0][2], col[1][2], col[2][2]]
    det = (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) + A[2] * (A[3] * A[7] - A[4] * A[6])
    if det < 0.0:
        A[2], A[5], A[8] = -A[2], -A[5], -A[8]
    return d, A


def shape_frame(points):
    """Rule C13 steps 1-4 for an (n, >= 3) float32 point set."""
    p = np.asarray(points, np.float32)
    p = np.ascontiguousarray((p if p.ndim == 2 else p.reshape(-1, 3))[:, :3])
    n = p.shape[0]
    if n > N_MAX:
        return ShapeFrame(n, CD_ERR_CAPACITY)
    if n and not bool(np.all(np.isfinite(p)) and np.all(np.abs(p) <= np.float32(COORD_MAX))):
        return ShapeFrame(n, CD_ERR_INVALID_ARG)
    if n < 3:
        return ShapeFrame(n, CD_ERR_FEW_CORRESPONDENCES)
    out = ShapeFrame(n)
    S = moments(p)
    fn = float(n)
    m = [(float(S[a]) * 2.0 ** -32) / fn for a in range(3)]
    e = [(float(S[3 + k]) * 2.0 ** -32) / fn for k in range(6)]
    c = [[0.0] * 3 for _ in range(3)]
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        c[a][b] = c[b][a] = e[k] - m[a] * m[b]
    out.mean = m
    out.var, out.axes = jacobi(c)
    A = out.axes
    pd = p.astype(np.float64)
    dx, dy, dz = pd[:, 0] - m[0], pd[:, 1] - m[1], pd[:, 2] - m[2]
    for a in range(3):
        q = (A[a] * dx + A[3 + a] * dy) + A[6 + a] * dz      # numpy float64: one IEEE operation per element, no contraction
        out.lo[a] = float(q.min()) + 0.0                     # (+ 0.0: a zero extent is stored as +0, whatever zero the reduction met first)
        out.hi[a] = float(q.max()) + 0.0
    return out


IDENTITY = np.eye(4, dtype=np.float32)


def guess(c, t):
    """Rule C13 step 5: (G 4x4 float32 scene -> template, flip index 0..3), or (identity, -1)."""
    if c.status != CD_OK or t.status != CD_OK:
        return IDENTITY.copy(), -1
    Ac, At, mc, mt = c.axes, t.axes, c.mean, t.mean
    sigma, w = [0.0] * 3, [0.0] * 3
    for a in range(3):
        s = t.lo[a] + t.hi[a]
        if abs(s) <= SIGMA_EPS * (t.hi[a] - t.lo[a]):
            sigma[a] = 0.0
        else:
            sigma[a] = 1.0 if -s > 0.0 else -1.0
        w[a] = -((Ac[a] * mc[0] + Ac[3 + a] * mc[1]) + Ac[6 + a] * mc[2])
    best, flip = 0.0, 0
    for k, F in enumerate(FLIPS):
        sc = ((F[0] * sigma[0]) * w[0] + (F[1] * sigma[1]) * w[1]) + (F[2] * sigma[2]) * w[2]
        if k == 0 or sc > best:          # the first candidate with the strictly largest score
            best, flip = sc, k
    F = FLIPS[flip]
    G = np.zeros(16, np.float64)
    for i in range(3):
        R = [((At[3 * i] * F[0]) * Ac[3 * j] + (At[3 * i + 1] * F[1]) * Ac[3 * j + 1]) + (At[3 * i + 2] * F[2]) * Ac[3 * j + 2]
             for j in range(3)]
        G[4 * i:4 * i + 3] = R
        G[4 * i + 3] = mt[i] - ((R[0] * mc[0] + R[1] * mc[1]) + R[2] * mc[2])
    G[15] = 1.0
    with np.errstate(over="ignore"):
        G32 = G.astype(np.float32)
    if not np.all(np.isfinite(G32)):
        return IDENTITY.copy(), -1
    return G32.reshape(4, 4), flip
