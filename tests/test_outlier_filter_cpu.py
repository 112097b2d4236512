"""Rule C16 (statistical outlier removal) without a GPU: the numpy module (perception_amd/outlier_filter.py) against a plain
Python loop and a hand-derived case, the host arithmetic of outlier_math.hpp (outlier_math_check, plain and sanitized) against the
module, the names the header and capi.py export, and synth.flying_pixels."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from perception_amd import capi, outlier_filter as OF, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_outlier_filter", "cd_get_outlier_filter", "cd_get_outlier_stats", "cd_outlier_filter"]


def test_header_and_capi_export_the_filter_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert re.search(r"#define CD_OUTLIER_MAX_MEAN_K %d\b" % OF.MAX_MEAN_K, header)
    assert re.search(r"#define CD_OUTLIER_LDS_TILE %d\b" % capi.CD_OUTLIER_LDS_TILE, header)
    assert capi.CD_OUTLIER_MAX_MEAN_K == OF.MAX_MEAN_K == 63
    assert re.search(r"#define CD_ABI_VERSION 4\b", header)


# ---- the clouds the CPU and the GPU tests share ---------------------------------------------------------------------------------
def random_cloud(n, seed, spread=0.1):
    """n points of a blob with a few far stragglers."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, spread, (n, 3))
    far = rng.random(n) < 0.05
    p[far] += rng.normal(0.0, 10.0 * spread, (int(far.sum()), 3))
    return p.astype(np.float32)


def lattice_cloud(side=6, pitch=0.0078125):
    """side^3 points on a lattice of a power-of-two pitch: the squared distances are exact, so the mean_k-th neighbour ties."""
    g = np.arange(side, dtype=np.float32) * np.float32(pitch)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def coincident_cloud(n=90, seed=3):
    """Every third point has a twin at its own coordinates, and one point has two."""
    p = random_cloud(n, seed)
    p[1::3] = p[0:-1:3][:len(p[1::3])]
    p[5] = p[4] = p[3]
    return p


def nan_cloud(n=70, seed=4):
    p = random_cloud(n, seed)
    p[7, 1] = np.nan
    p[20] = np.nan
    p[33, 2] = np.inf
    return p


# ---- the rule as a plain loop -----------------------------------------------------------------------------------------------------
def plain_filter(xyz, mean_k, std_mul, negative):
    """Sorted lists, one operation at a time with np.float32 and float; nothing shared with the module."""
    pts = [tuple(np.float32(v) for v in row[:3]) for row in np.asarray(xyz, np.float32)]
    fin = [all(math.isfinite(float(v)) for v in p) for p in pts]
    m = sum(fin)
    n = len(pts)
    dist = [np.float32(0.0)] * n
    if m <= mean_k:
        return [i for i in range(n) if fin[i]], dist, (0.0, 0.0, 0.0)
    with np.errstate(over="ignore"):
        for i in range(n):
            if not fin[i]:
                continue
            d2s = []
            for j in range(n):
                if not fin[j]:
                    continue
                dx = np.float32(pts[j][0] - pts[i][0])
                dy = np.float32(pts[j][1] - pts[i][1])
                dz = np.float32(pts[j][2] - pts[i][2])
                xx = np.float32(dx * dx)
                yy = np.float32(dy * dy)
                zz = np.float32(dz * dz)
                d2s.append(np.float32(np.float32(xx + yy) + zz))
            d2s.sort()
            best = d2s[:mean_k + 1]
            best.pop(0)
            s = 0.0
            for v in best:
                s = s + float(np.sqrt(np.float32(v)))
            dist[i] = np.float32(s / float(mean_k))
    total, sq = 0.0, 0.0
    for i in range(n):
        if fin[i]:
            d = float(dist[i])
            total = total + d
            sq = sq + d * d
    mean = total / float(m)
    var = (sq - total * total / float(m)) / float(m - 1)
    stddev = math.sqrt(var) if var >= 0.0 else float("nan")
    threshold = mean + float(std_mul) * stddev
    kept = []
    for i in range(n):
        if fin[i]:
            inlier = float(dist[i]) <= threshold
            if (not inlier) if negative else inlier:
                kept.append(i)
    return kept, dist, (mean, stddev, threshold)


def _bits64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _same(o, kept, dist, stats):
    assert o["indices"].dtype == np.int32 and list(o["indices"]) == list(kept)
    assert np.array_equal(o["dist"].view(np.uint32), np.array(dist, np.float32).view(np.uint32))
    assert [_bits64(o[k]) for k in ("mean", "stddev", "threshold")] == [_bits64(v) for v in stats]


PLAIN_CASES = [(5, 2, 1.0, False), (17, 16, 1.0, False), (18, 16, 1.0, False), (64, 1, 0.0, False), (65, 63, 1.0, True), (130, 16, 0.5, False),
               (200, 50, 1.0, False), (200, 8, -0.25, True)]


@pytest.mark.parametrize("n,mean_k,std_mul,negative", PLAIN_CASES)
def test_module_against_a_plain_loop(n, mean_k, std_mul, negative):
    p = random_cloud(n, 100 + n)
    _same(OF.outlier_filter(p, mean_k, std_mul, negative), *plain_filter(p, mean_k, std_mul, negative))


@pytest.mark.parametrize("make,mean_k", [(lattice_cloud, 6), (lattice_cloud, 16), (coincident_cloud, 4), (nan_cloud, 10)])
def test_module_against_a_plain_loop_on_ties_twins_and_nan(make, mean_k):
    p = make() if make is not lattice_cloud else make(4)
    for negative in (False, True):
        _same(OF.outlier_filter(p, mean_k, 1.0, negative), *plain_filter(p, mean_k, 1.0, negative))


def test_hand_derived_collinear_case():
    """Ten collinear points 1 cm apart and one 0.5 m away, mean_k = 2, std_mul = 1: the end points' two nearest neighbours are 1
    and 2 cm away (mean 1.5 cm), the inner points' 1 and 1 cm; the far point's mean distance is about half a metre and it alone is
    beyond mean + stddev."""
    p = np.zeros((11, 3), np.float32)
    p[:10, 0] = np.arange(10) * 0.01
    p[10] = (0.045, 0.5, 0.0)
    o = OF.outlier_filter(p, 2, 1.0)
    assert list(o["indices"]) == list(range(10)) and o["computed"] and o["n_finite"] == 11
    assert np.allclose(o["dist"][[0, 9]], 0.015, rtol=1e-5) and np.allclose(o["dist"][1:9], 0.01, rtol=1e-5)
    assert 0.5 < o["dist"][10] < 0.51 and o["dist"][10] > o["threshold"] > 0.015
    assert list(OF.outlier_filter(p, 2, 1.0, negative=True)["indices"]) == [10]
    kept, rec = OF.filter_cloud(np.concatenate([p, np.arange(11, dtype=np.float32)[:, None]], 1), 2, 1.0)
    assert list(kept[:, 3]) == list(range(10)) and rec["n_finite"] == 11


def test_small_clouds_and_arguments():
    p = random_cloud(16, 9)
    p[3, 0] = np.nan
    for negative in (False, True):                 # m = 15 <= mean_k = 15: every finite point, nothing computed
        o = OF.outlier_filter(p, 15, 1.0, negative)
        assert list(o["indices"]) == [i for i in range(16) if i != 3] and not o["computed"]
        assert (o["mean"], o["stddev"], o["threshold"]) == (0.0, 0.0, 0.0) and not o["dist"].any()
    assert OF.outlier_filter(p, 14, 1.0)["computed"]
    assert OF.outlier_filter(np.zeros((0, 3), np.float32), 1, 1.0)["indices"].shape == (0,)
    for bad in (0, 64, -1):
        with pytest.raises(ValueError):
            OF.outlier_filter(p, bad, 1.0)
    with pytest.raises(ValueError):
        OF.outlier_filter(p, 4, float("nan"))


# ---- outlier_math.hpp on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("outlier") / "outlier_math_check")
    cmd = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
           "-Wno-unknown-pragmas"] + ([request.param] if request.param else []) + [os.path.join(CSRC, "outlier_math_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run_check(exe, tmp_path, p, mean_k, std_mul, negative):
    path = str(tmp_path / "cloud.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiiid", len(p), mean_k, 1 if negative else 0, 0, std_mul))
        fp.write(np.ascontiguousarray(p, "<f4").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    n, m, computed, kept = (int(v) for v in lines["counts"].split())
    dist = np.array([int(v, 16) for v in lines["dist"].split()], np.uint32)
    stats = [int(v, 16) for v in lines["stats"].split()]
    flags = np.array([c == "1" for c in lines["kept"].strip()], bool)
    return n, m, computed, kept, dist, stats, flags


CHECK_CASES = [("random", lambda: random_cloud(300, 11), 16, 1.0, False), ("random_k63", lambda: random_cloud(129, 12), 63, 0.0, False),
               ("lattice", lattice_cloud, 16, 1.0, False), ("lattice_negative", lattice_cloud, 6, 1.0, True),
               ("coincident", coincident_cloud, 4, 1.0, False), ("nan", nan_cloud, 10, 1.0, False), ("small", lambda: random_cloud(8, 13), 8, 1.0, True)]


@pytest.mark.parametrize("name,make,mean_k,std_mul,negative", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_outlier_math_on_the_host(check_exe, tmp_path, name, make, mean_k, std_mul, negative):
    p = make()
    o = OF.outlier_filter(p, mean_k, std_mul, negative)
    n, m, computed, kept, dist, stats, flags = _run_check(check_exe, tmp_path, p, mean_k, std_mul, negative)
    assert (n, m, bool(computed), kept) == (len(p), o["n_finite"], o["computed"], len(o["indices"]))
    assert np.array_equal(dist, o["dist"].view(np.uint32))
    assert stats == [_bits64(o[k]) for k in ("mean", "stddev", "threshold")]
    assert np.array_equal(np.flatnonzero(flags), o["indices"])
    if name.startswith("lattice"):     # the case is about ties at the mean_k-th neighbour: most points have one
        d2 = np.sort(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1), axis=1)
        assert (d2[:, mean_k] == d2[:, mean_k + 1]).sum() > len(p) // 2


def test_check_program_refuses_bad_arguments(check_exe, tmp_path):
    path = str(tmp_path / "bad.bin")
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iiiid", 4, 64, 0, 0, 1.0) + np.zeros(12, "<f4").tobytes())
    assert subprocess.run([check_exe, path], capture_output=True).returncode == 2


# ---- synth.flying_pixels ---------------------------------------------------------------------------------------------------------------
def test_flying_pixels_moves_edge_pixels_along_their_rays():
    w, h = 320, 240
    rec = synth.frame(0, width=w, height=h)
    out = synth.flying_pixels(rec, w, h, seed=5, frac=0.5)
    assert out.shape == rec.shape and out.dtype == np.float32 and out is not rec
    assert np.array_equal(synth.flying_pixels(rec, w, h, seed=5, frac=0.5).view(np.uint32), out.view(np.uint32))      # a pure function
    assert np.array_equal(synth.flying_pixels(rec, w, h, seed=5, frac=0.0).view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(out[:, 3].view(np.uint32), rec[:, 3].view(np.uint32))                                        # colours stay
    changed = np.flatnonzero((out[:, :3].view(np.uint32) != rec[:, :3].view(np.uint32)).any(1))
    assert len(changed) > 20
    z0, z1 = rec[changed, 2].astype(np.float64), out[changed, 2].astype(np.float64)
    assert np.isfinite(z0).all() and np.isfinite(z1).all()
    for a in (0, 1):                                    # along the ray: x / z and y / z stay
        assert np.allclose(out[changed, a] / z1, rec[changed, a] / z0, atol=1e-5)
    zi = rec[:, 2].reshape(h, w).astype(np.float64)
    for i in changed[:200]:                             # on a jump of more than 1 cm, and between its two sides
        v, u = divmod(int(i), w)
        nb = [zi[v, u + d] for d in (-1, 1) if 0 <= u + d < w] + [zi[v + d, u] for d in (-1, 1) if 0 <= v + d < h]
        nb = [z for z in nb if np.isfinite(z) and abs(z - zi[v, u]) > 0.01]
        assert nb
        assert any(min(z, zi[v, u]) - 1e-6 <= out[i, 2] <= max(z, zi[v, u]) + 1e-6 for z in nb)
