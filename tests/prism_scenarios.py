"""Inputs of the table-prism tests (rule C20), CPU only: integer point sets placed on the plane z = 0, where a point
((i + 0.5) / 65536, (j + 0.5) / 65536, z) is exact in float32, quantises to (i, j) and has the height z; and the finite-table
scenes - a frame of the synthetic sequence whose table is cut to a rectangle, with a second cuboid floating beside it."""
import numpy as np

from perception_amd import capi, synth

COEFF_Z = np.array([0.0, 0.0, 1.0, 0.0], np.float32)


def xyz_of_uv(uv, z=0.0):
    """(n, 3) float32 points of the plane z = 0 (or at height z, a scalar or (n,)) that quantise to the integer (u, v)."""
    a = np.asarray(uv, np.int64).reshape(-1, 2)
    p = np.zeros((len(a), 3), np.float32)
    p[:, :2] = ((a.astype(np.float64) + 0.5) / 65536.0).astype(np.float32)
    p[:, 2] = z
    assert np.array_equal(np.floor(p[:, :2].astype(np.float64) * 65536.0).astype(np.int64), a), "not exact in float32"
    return p


def case(plane_uv, uv, z=0.01, limits=(0.0, 0.5), coeff=COEFF_Z):
    return dict(plane=xyz_of_uv(plane_uv), coeff=np.asarray(coeff, np.float32), xyz=xyz_of_uv(uv, z), limits=limits)


SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10)]
PROBES = [(5, 5), (5, 0), (10, 5), (10, 10), (0, 0), (11, 5), (-1, -1), (5, 11), (0, 10), (3, 7)]   # inside, on edges, on vertices, outside


def small_cases():
    """name -> case: the tiny and degenerate sets."""
    rng = np.random.RandomState(20)
    interior = [(int(a), int(b)) for a, b in rng.randint(1, 10, (40, 2))]
    out = {}
    out["square"] = case(SQUARE + interior, PROBES)
    out["collinear_and_duplicates"] = case(SQUARE + [(5, 0), (10, 5), (5, 10), (0, 5), (0, 0), (10, 10), (10, 10)] + interior, PROBES)
    out["all_collinear"] = case([(i, 2 * i) for i in range(-5, 9)], PROBES + [(1, 2), (8, 16)])
    out["no_inlier"] = case([], PROBES)
    out["one_inlier"] = case([(5, 5)], PROBES)
    out["two_inliers"] = case([(0, 0), (10, 10)], PROBES)
    out["one_point_many_times"] = case([(5, 5)] * 70, PROBES)
    out["triangle"] = case([(0, 0), (7, 1), (3, 9)], PROBES + [(3, 3), (7, 1), (5, 5), (2, 6)])
    z = np.array([0.0, 0.02, 0.05, np.nextafter(np.float32(0.02), np.float32(0)), np.nextafter(np.float32(0.05), np.float32(1)), -0.01, 0.3, np.nan, 0.03, 0.04],
                 np.float32)
    out["heights"] = case(SQUARE, [(5, 5)] * 10, z=z, limits=(float(np.float32(0.02)), float(np.float32(0.05))))
    out["no_object_point"] = case(SQUARE, [])
    return out


def grid_case(n, seed, span=8):
    """n plane points drawn from a span x span integer grid (collinearity and duplicates everywhere), probes all over and around it."""
    rng = np.random.RandomState(seed)
    plane = rng.randint(0, span, (n, 2))
    probes = rng.randint(-2, span + 2, (300, 2))
    return case(plane, probes, z=(rng.randint(0, 4, 300) * 0.01).astype(np.float32), limits=(0.01, 0.02))


def wide_grid_case(n, seed, span=2000):
    rng = np.random.RandomState(seed)
    plane = rng.randint(-span, span, (n, 2))
    probes = rng.randint(-span - 100, span + 100, (1500, 2))
    return case(plane, probes)


def circle_case(n=5000, radius=0.4):
    """n points on a circle of `radius` metres: none is strictly inside the polygon of the eight extremes."""
    t = 2.0 * np.pi * np.arange(n) / n
    uv = np.floor(np.stack([np.cos(t), np.sin(t)], 1) * radius * 65536.0).astype(np.int64)
    rng = np.random.RandomState(5)
    r = int(radius * 65536.0)
    probes = rng.randint(-r - 50, r + 50, (2000, 2))
    return case(uv, np.r_[probes, uv[::97]])


def parabola_case(n):
    """u = i, v = i^2: every point is a strict hull vertex."""
    i = np.arange(n, dtype=np.int64)
    uv = np.stack([i, i * i], 1)
    return case(uv, [(10, 200), (500, 300000), (0, 0), (n - 1, (n - 1) ** 2), (-1, 0), (100, 9999), (100, 10000)])


def edge_case():
    """object points exactly on the edges and vertices of a hull with slanted edges, and their neighbours one unit outside"""
    hull = [(0, 0), (12, 4), (16, 16), (4, 12)]
    on = [(3, 1), (6, 2), (9, 3), (13, 7), (14, 10), (15, 13), (1, 3), (2, 6), (3, 9), (10, 14), (7, 13)] + hull
    off = [(3, 0), (6, 1), (13, 6), (16, 13), (0, 3), (2, 7), (10, 15), (-1, 0), (17, 16)]
    return case(hull + [(8, 8)], on + off)


# ---- the finite-table scenes -----------------------------------------------------------------------------------------------------
TABLE_HALF = (0.18, 0.25)          # the table's extent along e1 and e2 around p0
FLOAT_AT, FLOAT_UP = 0.33, 0.06    # the second cuboid: along e1 from p0, its underside above the plane level


def finite_table_params():
    prm = capi.default_params()
    prm.crop_x_min, prm.crop_x_max = -0.5, 0.5
    return prm


def finite_table_scene(index):
    sc = synth.scene_for(index, k_obj=1)
    L, W, H = synth.CUBOID_DIMS
    n, e1, e2, p0 = sc["n"], sc["e1"], sc["e2"], sc["p0"]
    sc["boxes"].append(dict(R=np.stack([e1, np.cross(n, e1), n], axis=1), c=p0 + FLOAT_AT * e1 + (FLOAT_UP + H / 2.0) * n,
                            half=np.array([L, W, H]) / 2.0, yaw=0.0))
    return sc


def finite_table_frame(index):
    """Frame `index` with one cuboid on a table cut to TABLE_HALF (beyond it there is nothing: NaN) and a second cuboid floating
    beside the table, FLOAT_UP above the plane level: (640 * 480, 4) float32 records."""
    sc = finite_table_scene(index)
    rec = synth.render(sc)
    table = rec[:, 3].view(np.uint32) == synth._pack_rgb(150, 140, 130)
    d = rec[:, :3].astype(np.float64) - sc["p0"]
    with np.errstate(invalid="ignore"):
        off = table & ((np.abs(d @ sc["e1"]) > TABLE_HALF[0]) | (np.abs(d @ sc["e2"]) > TABLE_HALF[1]))
    rec[off, :3] = np.nan
    return rec


# ---- the scenarios of the fused-call tests: name -> (frames, cd_params, (height_min, height_max), cache keys) ---------------------
_FRAMES = {}


def scenario(name):
    """'a': frames 0..15 at the default parameters, limits (0, 0.5) - the step removes nothing.  'b': the finite-table scenes of
    frames 0, 3 and 7 - two clusters become one.  'c': frames 0..7 with height_max 0.025 - the step cuts the cuboids' tops off."""
    if name not in _FRAMES:
        if name == "b":
            _FRAMES[name] = [finite_table_frame(i) for i in (0, 3, 7)]
        else:
            _FRAMES[name] = [synth.frame(i) for i in range(16 if name == "a" else 8)]
    frames = _FRAMES[name]
    prm = finite_table_params() if name == "b" else capi.default_params()
    prm.rgb_offset = 12          # (the colour travels with the point)
    limits = (0.0, 0.025) if name == "c" else (0.0, 0.5)
    keys = [("table", i) for i in (0, 3, 7)] if name == "b" else [("synth", i) for i in range(len(frames))]
    return frames, prm, limits, keys
