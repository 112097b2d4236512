"""Rule C22 (reciprocal correspondences) without a GPU: the numpy module (perception_amd/icp_reciprocal.py) on known answers and
against the oracle's nearest neighbours composed in both directions, the host arithmetic of icp_recip_math.hpp
(icp_recip_math_check, plain and sanitized, and cd_icp_reciprocal_mask) against the module bit for bit, the reference pair
(tests/recip_reference.py) against the oracle's ICP when nothing is rejected, every precondition of the GPU scenarios
(tests/recip_scenarios.py) from the reference alone, the stage planning with the mode on, and the names the header, capi.py and the
PCL mirror export."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fused_reference as FR
import recip_reference as QR
import recip_scenarios as S
import reject_reference as RR
from oracle import oracle_py as O
from perception_amd import capi, cluster_frame as cf, icp_coarse as IC, icp_reciprocal as IQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_icp_reciprocal", "cd_get_icp_reciprocal", "cd_icp_recip_struct_size", "cd_get_cluster_recip_stats", "cd_icp_reciprocal_mask"]
f32, f64 = np.float32, np.float64
HOST_CXX = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas"]


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS, name
    body = re.search(r"typedef struct cd_icp_recip_stats \{(.*?)\} cd_icp_recip_stats;", header, re.S).group(1)
    fields = re.findall(r"\b(int32_t)\s+(\w+)(\[3\])?;", body)
    assert [(n, bool(a)) for _, n, a in fields] == [("first_kept", False), ("last_kept", False), ("min_kept", False), ("stopped_few", False),
                                                   ("last_n0", False), ("reserved", True)]
    assert [n for n, _ in capi.CdIcpRecipStats._fields_] == [n for _, n, _ in fields]
    assert C.sizeof(capi.CdIcpRecipStats) == 32
    assert "setUseReciprocalCorrespondences" in header and "unpinned" in header
    for fn in (capi.Context.set_icp_reciprocal, capi.Context.icp_reciprocal, capi.Context.cluster_recip_stats, capi.icp_reciprocal_mask):
        assert callable(fn)


def test_pcl_compat_has_the_switch(tmp_path):
    src = str(tmp_path / "reciprocal.cpp")
    open(src, "w").write("""#include "pcl_compat.hpp"
namespace pcl = pclhip;
int main() {
    pcl::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
    if (icp.getUseReciprocalCorrespondences()) return 1;
    icp.setUseReciprocalCorrespondences(true);
    return icp.getUseReciprocalCorrespondences() ? 0 : 1;
}
""")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "perception_amd", "cpp"), src], check=True)
    text = open(os.path.join(ROOT, "perception_amd", "cpp", "pcl_compat.hpp")).read()
    assert re.search(r"cd_set_icp_reciprocal\(Device::instance\(\)\.ctx\(\), reciprocal_ \? 1 : 0\)", text)


# ---- the module on known answers -----------------------------------------------------------------------------------------------------
TPL9 = np.array([[x, y, 0.0] for x in (0.0, 0.1, 0.2) for y in (0.0, 0.1, 0.2)], f32)


def mask(src, tpl, d2_max=None):
    src = np.ascontiguousarray(src, f32)
    nn, d2 = IQ.forward(src, tpl)
    keep, n0 = IQ.keep_mask(src, tpl, nn, d2, d2_max)
    return keep, n0, nn, d2


def test_module_ties_go_to_the_lower_index():
    delta = f32(2.0 ** -8)
    q = TPL9[4]
    pair = np.array([q + [0, 0, delta], q - [0, 0, delta]], f32)
    others = TPL9[[0, 8]] + f32(0.001)
    for a, b in ((0, 1), (1, 0)):
        src = np.vstack([pair[[a, b]], others])
        keep, n0, nn, d2 = mask(src, TPL9)
        assert nn[:2].tolist() == [4, 4] and d2[:2].view(np.uint32)[0] == d2[:2].view(np.uint32)[1] and d2[0] > 0
        assert keep.tolist() == [True, False, True, True] and n0 == 4
    # three at the same distance bits: only the first
    src = np.vstack([q + [0, 0, delta], q - [0, 0, delta], q + [delta, 0, 0], others])
    assert mask(src, TPL9)[0].tolist() == [True, False, False, True, True]


def test_module_duplicates_keep_the_lower_index():
    base = TPL9[[0, 2, 4, 6, 8]] + np.array([0.002, -0.001, 0.003], f32)
    src = np.vstack([base, base[[1, 3]], base[[1]]])
    keep, n0, _, _ = mask(src, TPL9)
    assert keep.tolist() == [True] * 5 + [False] * 3 and n0 == 8


def test_module_ball_beyond_a_corner_keeps_one():
    rng = np.random.default_rng(3)
    ball = (TPL9[8] + 0.05 + rng.normal(scale=0.001, size=(30, 3))).astype(f32)
    keep, n0, nn, d2 = mask(ball, TPL9)
    assert (nn == 8).all() and keep.sum() == 1 and keep[np.argmin(d2)] and n0 == 30
    assert int(np.flatnonzero(keep)[0]) == int(np.flatnonzero(d2 == d2.min())[0])


def test_module_bound_and_small_k0():
    src = np.vstack([TPL9[[0, 4, 8]] + f32(0.001), TPL9[[2]] + f32(0.04)]).astype(f32)
    keep, n0, _, d2 = mask(src, TPL9)
    assert keep.all() and n0 == 4
    keep, n0, _, _ = mask(src, TPL9, d2_max=f32(1e-4))
    assert keep.tolist() == [True, True, True, False] and n0 == 3
    # the far point takes no part in K0 but is a target of the reverse search: put it nearest to a near point's template point
    src2 = np.vstack([TPL9[[0, 4, 8]] + f32(0.02), TPL9[[4]] + np.array([0.0, 0.0, 0.001], f32)]).astype(f32)
    keep, n0, nn, d2 = mask(src2, TPL9, d2_max=f32(np.sort(IQ.forward(src2, TPL9)[1])[0]))
    assert n0 == 1 and keep.sum() == 1                       # |K0| < 3: K0 itself
    keep, n0, nn, d2 = mask(src2, TPL9, d2_max=None)
    assert nn.tolist() == [0, 4, 8, 4] and keep.tolist() == [True, False, True, True]
    bound = f32(d2[:3].max())
    far_first = np.vstack([src2[[3]] + np.array([0, 0, 0.05], f32), src2[:3], src2[[3]]]).astype(f32)   # index 0: beyond the bound, nearest to nothing
    keep, n0, nn, d2 = mask(far_first, TPL9, d2_max=bound)
    assert n0 == 4 and keep.tolist() == [False, True, False, True, True]
    # two points in K0: the caller stops, nothing is tested
    keep, n0, _, _ = mask(src[:2], TPL9)
    assert keep.all() and n0 == 2


@pytest.mark.parametrize("kind", S.KINDS)
def test_module_equals_the_oracle_composed_in_both_directions(kind):
    tpl = S.template(kind)
    sources = [RR.contamination_scene(tpl, 2)[0], S.duplicate_source(kind)[0], S.corner_ball(kind), S.sized_source(kind, 513, 513)]
    if kind == "lattice":
        sources.append(S.tie_source()[0])
    for src in sources:
        nn, d2 = O.nn(tpl, src, mode=1)
        for bound in (None, f32(np.quantile(d2.astype(f64), 0.7))):
            keep, n0 = IQ.keep_mask(src, tpl, nn, d2, bound)
            assert np.array_equal(keep, QR.keep_by_oracle(tpl, src, nn, d2, bound))
            assert n0 == int((d2 <= (bound if bound is not None else np.inf)).sum())
        fn, fd = IQ.forward(src, tpl)
        assert np.array_equal(fd.view(np.uint32), d2.view(np.uint32)) and np.array_equal(tpl[fn], tpl[nn])


# ---- the host arithmetic of icp_recip_math.hpp -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_recip") / "icp_recip_math_check")
    subprocess.run(HOST_CXX + ([request.param] if request.param else []) + [os.path.join(CSRC, "icp_recip_math_check.cpp"), "-o", exe], check=True)
    return exe


def host_cases():
    """[(src, tpl, bound or None, note)]"""
    out = []
    delta = f32(2.0 ** -8)
    q = TPL9[4]
    out.append((np.vstack([q - [0, 0, delta], q + [0, 0, delta], TPL9[[0, 8]] + f32(0.001)]), TPL9, None, "tie"))
    base = TPL9[[0, 2, 4, 6, 8]] + np.array([0.002, -0.001, 0.003], f32)
    out.append((np.vstack([base, base[[1, 3]]]), TPL9, None, "duplicates"))
    rng = np.random.default_rng(3)
    out.append(((TPL9[8] + 0.05 + rng.normal(scale=0.001, size=(30, 3))), TPL9, None, "corner ball"))
    out.append((TPL9[[1, 5]] + f32(0.003), TPL9, None, "two points"))
    out.append((TPL9[[1]] + f32(0.003), TPL9[[3]], None, "one and one"))
    for kind in S.KINDS:
        tpl = S.template(kind)
        src = S.sized_source(kind, 257, 257)
        d2 = IQ.forward(src, tpl)[1]
        out.append((src, tpl, None, kind + " sized"))
        out.append((src, tpl, f32(np.quantile(d2.astype(f64), 0.6)), kind + " sized bounded"))
        out.append((src, tpl, f32(0.0), kind + " bound 0"))
        out.append((S.duplicate_source(kind, 120, 50)[0], tpl, None, kind + " duplicates"))
    out.append((S.tie_source(60)[0], S.template("lattice"), None, "lattice ties"))
    return [(np.ascontiguousarray(s, f32), np.ascontiguousarray(t, f32), b, note) for s, t, b, note in out]


def test_check_program_equals_the_module_bitwise(check_exe, tmp_path):
    for i, (src, tpl, bound, note) in enumerate(host_cases()):
        path = str(tmp_path / ("case%d.bin" % i))
        with open(path, "wb") as fp:
            fp.write(struct.pack("<iiif", len(src), len(tpl), 0 if bound is None else 1, 0.0 if bound is None else float(bound)) + src.astype("<f4").tobytes() +
                     tpl.astype("<f4").tobytes())
        r = subprocess.run([check_exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (note, r.stdout + r.stderr)
        lines = r.stdout.strip().split("\n")
        nn, d2 = IQ.forward(src, tpl)
        keep, n0 = IQ.keep_mask(src, tpl, nn, d2, bound)
        assert lines[0].split() == ["counts", str(len(src)), str(n0), str(int(keep.sum()))], note
        assert [int(v) for v in lines[1].split()[1:]] == nn.tolist(), note
        assert lines[2] == "d2 " + "".join("%08x" % v for v in d2.view(np.uint32)), note
        assert lines[3] == "keep " + "".join("1" if k else "0" for k in keep), note
    bad = str(tmp_path / "bad.bin")
    with open(bad, "wb") as fp:
        fp.write(struct.pack("<iiif", 0, 3, 0, 0.0))
    assert subprocess.run([check_exe, bad], capture_output=True).returncode == 2


def test_library_struct_size_and_host_mask():
    lib = capi.load_library()
    assert lib.cd_icp_recip_struct_size() == C.sizeof(capi.CdIcpRecipStats)
    for src, tpl, bound, note in host_cases():
        nn, d2, keep, n0 = capi.icp_reciprocal_mask(src, tpl, bound)
        en, ed = IQ.forward(src, tpl)
        ek, en0 = IQ.keep_mask(src, tpl, en, ed, bound)
        assert np.array_equal(nn, en) and np.array_equal(d2.view(np.uint32), ed.view(np.uint32)) and np.array_equal(keep, ek) and n0 == en0, note
    src, tpl = host_cases()[0][:2]
    for bad in (float("nan"), -1.0):
        with pytest.raises(capi.CuboidError) as ei:
            capi.icp_reciprocal_mask(src, tpl, bad)
        assert ei.value.status == capi.CD_ERR_INVALID_ARG
    keep = np.zeros(len(src), np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.cd_icp_reciprocal_mask(vp(src), 12, len(src), vp(tpl), 12, len(tpl), float("inf"), None, None, vp(keep)) == len(src)   # nn, d2 may be NULL
    assert lib.cd_icp_reciprocal_mask(vp(src), 10, len(src), vp(tpl), 12, len(tpl), float("inf"), None, None, vp(keep)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_icp_reciprocal_mask(vp(src), 12, 0, vp(tpl), 12, len(tpl), float("inf"), None, None, vp(keep)) == capi.CD_ERR_INVALID_ARG
    assert lib.cd_icp_reciprocal_mask(vp(src), 12, len(src), vp(tpl), 12, len(tpl), float("inf"), None, None, None) == capi.CD_ERR_INVALID_ARG


# ---- the stage planning with the mode on -------------------------------------------------------------------------------------------
PLAN_MAIN = r"""
#include <cstdio>
#include "icp_plan.hpp"
using namespace cd;
// 60 clusters of a lattice template and of a gridded one, and one of two points; argv: recip_on reject_on plane_on
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    std::vector<IcpCluster> cl;
    for (int k = 0; k < 60; ++k) cl.push_back(IcpCluster{k * 1024, 100 + k, k / 8, k % 8, 0, 1700, 0, 0});
    cl.push_back(IcpCluster{60 * 1024, 2, 7, 4, 0, 1700, 0, 0});
    for (int k = 0; k < 60; ++k) cl.push_back(IcpCluster{(61 + k) * 1024, 700 + k, k / 8, k % 8, 1700, 2979, 0, 1});
    const int faces[CD_MAX_TEMPLATES] = {3, 0};
    const bool gridded[CD_MAX_TEMPLATES] = {true, true}, big[CD_MAX_TEMPLATES] = {false, false};
    Tunables tun = Tunables();
    IcpPlanInput in;
    in.cl = cl.data(); in.ncl = (int)cl.size();
    in.tpl_faces = faces; in.tpl_gridded = gridded; in.tpl_big = big;
    in.tun = &tun; in.n_cu = 256; in.work_cap = 1 << 16;
    in.recip_on = argv[1][0] == '1'; in.reject_on = argv[2][0] == '1'; in.plane_on = argv[3][0] == '1';
    std::vector<IcpWork> work((size_t)in.work_cap);
    std::vector<IcpState> st(2 * cl.size());
    IcpPlan pl;
    const PlanStatus ps = plan_icp(in, &pl, work.data(), st.data());
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", ps.code, (int)pl.recip, (int)pl.filtered(), pl.n_lat, (int)pl.grouped_pipe, (int)pl.whole_cluster, (int)pl.lat_direct,
                pl.icp_search, pl.nwork, pl.qslice, pl.n_live, cl[60].tile0 == cl[61].tile0);
    if (ps.msg) std::printf("%s\n", ps.msg);
    return 0;
}
"""


def test_plan_with_the_mode_on_is_all_sliced(tmp_path):
    tun = open(os.path.join(CSRC, "tunables.hpp")).read()
    src, exe = str(tmp_path / "plan_recip.cpp"), str(tmp_path / "plan_recip")
    open(src, "w").write(PLAN_MAIN)
    assert "struct Tunables" in tun
    subprocess.run(HOST_CXX + ["-I" + CSRC, src, "-o", exe], check=True)

    def plan(recip, reject=0, plane=0):
        r = subprocess.run([exe, str(recip), str(reject), str(plane)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().split("\n")
        return [int(v) for v in lines[0].split()], lines[1:]
    off, _ = plan(0)
    assert off[0] == 0 and off[1:3] == [0, 0] and off[3] == 60 and (off[4] or off[5] or off[8] == 0)
    on, _ = plan(1)
    code, recip, filtered, n_lat, grouped, whole, direct, search, nwork, q, n_live, no_items = on
    assert (code, recip, filtered, n_lat, grouped, whole, direct, search) == (0, 1, 1, 0, 0, 0, 0, 0)
    assert nwork == sum(-(-(100 + k) // q) for k in range(60)) + sum(-(-(700 + k) // q) for k in range(60)) and n_live == 120 and no_items == 1
    for reject, plane in ((1, 0), (0, 1)):
        both, msg = plan(1, reject, plane)
        assert both[0] == capi.CD_ERR_INVALID_ARG and "both on" in msg[0]


# ---- the reference pair --------------------------------------------------------------------------------------------------------------
def oracle_pair(tpl, src, prm, guess=None):
    q = FR.copy_params(prm)
    q.icp_use_guess = capi.CD_GUESS_NONE
    if guess is not None:
        q.icp_use_guess = capi.CD_GUESS_PARAMS
        q.icp_guess[:] = [float(v) for v in np.asarray(guess, f32).ravel()]
    st, r, al = O.icp(tpl, src, q, nn_mode=1, want_aligned=True)
    assert st == 0
    return r, al


def bits64(v):
    return int(np.array([v], f64).view(np.uint64)[0])


def same_as_oracle(e, r, al):
    assert e["T"].view(np.uint32).ravel().tolist() == np.array(list(r.T), f32).view(np.uint32).tolist()
    assert (e["iterations"], e["converged"], e["accepted"]) == (r.iterations, r.converged, r.accepted) and bits64(e["fitness"]) == bits64(r.fitness)
    assert np.array_equal(e["aligned"].view(np.uint32), al.view(np.uint32))


@pytest.mark.parametrize("kind", S.KINDS)
def test_reference_pair_equals_the_oracle_when_nothing_is_rejected(kind):
    tpl, prm = S.template(kind), S.icp_params()
    assert len(tpl) == {"lattice": 1700, "scanned": 2979}[kind]
    # distinct template points as the source: every point is its template point's nearest source, at distance 0
    src = S.exact_subset(kind)
    e = QR.pair(tpl, src, prm)
    same_as_oracle(e, *oracle_pair(tpl, src, prm))
    assert e["kept"] == [len(src)] * len(e["kept"]) and e["recip_stats"] == QR.RecipStats(len(src), len(src), len(src), 0, len(src))
    # ... and the composition with the rule off on the contamination scene, with and without a guess
    src, _ = RR.contamination_scene(tpl, 2)
    for guess in (None, np.array(cf.guess(cf.shape_frame(src), cf.shape_frame(tpl))[0], f32)):
        e = QR.pair(tpl, src, prm, guess=guess, on=False)
        same_as_oracle(e, *oracle_pair(tpl, src, prm, guess))
        assert e["iterations"] > 3


# ---- the preconditions of the GPU scenarios -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_contamination_scene_is_helped_by_the_rule(kind):
    tpl, prm = S.template(kind), S.icp_params()
    for seed in S.SCENE_SEEDS:
        src, truth = RR.contamination_scene(tpl, seed)
        assert len(src) == 1800
        r, _ = oracle_pair(tpl, src, prm)
        on = QR.pair(tpl, src, prm)
        err_off = RR.translation_error(np.array(list(r.T)).reshape(4, 4), truth)
        err_on = RR.translation_error(on["T"], truth)
        assert err_on < 0.5 * err_off, (kind, seed, err_on, err_off)
        assert on["converged"] and len(set(on["kept"])) > 1 and on["recip_stats"].min_kept < 1500      # the kept counts change over the iterations
    assert S.SCENE_SEEDS == (2, 3, 4, 5) and set(S.GPU_SCENE_SEEDS) <= set(S.SCENE_SEEDS)


@pytest.mark.parametrize("kind", S.KINDS)
def test_sized_sources_cover_the_paths(kind):
    tpl, prm = S.template(kind), S.icp_params()
    assert S.SIZES == (3, 4, 5, 10, 14, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 4099)
    assert S.SPLIT_SIZE > 3 * S.RC_CHUNK and S.SPLIT_SIZE % S.RC_CHUNK not in (0, 1)
    varied = 0
    for n in S.SIZES + (S.SPLIT_SIZE,):
        src = S.sized_source(kind, n, n) if n != S.SPLIT_SIZE else S.split_source(kind)
        assert len(src) == n
        e = QR.pair(tpl, src, prm)
        assert e["converged"] and not e["stopped"] and e["iterations"] >= 2, n
        if n >= 63:
            assert 3 <= e["recip_stats"].min_kept < n, n       # something is rejected
        varied += len(set(e["kept"])) > 1
    assert varied >= 6


def test_tie_and_duplicate_sources():
    prm = S.icp_params()
    tpl = S.template("lattice")
    src, pts = S.tie_source()
    nn, d2 = O.nn(tpl, src, mode=1)
    assert np.array_equal(d2[0::2].view(np.uint32), d2[1::2].view(np.uint32)) and (d2 > 0).all() and np.array_equal(tpl[nn[0::2]], pts) and np.array_equal(nn[0::2], nn[1::2])
    keep, _ = IQ.keep_mask(src, tpl, nn, d2)
    assert keep[0::2].all() and not keep[1::2].any()
    w = int(np.flatnonzero(src[0] != src[1])[0])
    assert (np.sign(src[0::2, w] - src[1::2, w])[0::2] != np.sign(src[0::2, w] - src[1::2, w])[1::2]).all()   # the kept point is outside for even pairs, inside for odd ones
    e = QR.pair(tpl, src, prm)
    assert e["kept"][0] == len(pts) and e["converged"]
    for kind in S.KINDS:
        tpl = S.template(kind)
        src, pick = S.duplicate_source(kind)
        n = len(src) - len(pick)
        assert np.array_equal(src[n:], src[pick])
        nn, d2 = O.nn(tpl, src, mode=1)
        keep, _ = IQ.keep_mask(src, tpl, nn, d2)
        assert not keep[n:].any() and keep[pick].any()
        e = QR.pair(tpl, src, prm)
        assert e["converged"] and max(e["kept"]) <= n and e["iterations"] >= 2


@pytest.mark.parametrize("kind", S.KINDS)
def test_stop_scenarios_stop(kind):
    tpl, prm = S.template(kind), S.icp_params()
    src = S.corner_ball(kind)
    e = QR.pair(tpl, src, prm)
    assert len(src) == 40 and e["kept"] == [1] and (e["iterations"], e["converged"], e["accepted"], e["stopped"]) == (0, 0, 0, 1)
    assert np.array_equal(e["T"], np.eye(4, dtype=f32)) and np.array_equal(e["aligned"], src) and e["recip_stats"] == QR.RecipStats(1, 1, 1, 1, 40)
    later = QR.pair(tpl, S.stops_later(kind), prm)
    assert later["stopped"] and later["iterations"] >= 1 and not later["converged"] and later["kept"][-1] < 3 and min(later["kept"][:-1]) >= 3
    assert not np.array_equal(later["T"], np.eye(4, dtype=f32))                         # Tfinal as it stood at the stop


@pytest.mark.parametrize("kind", S.KINDS)
def test_bound_scenarios(kind):
    tpl, prm = S.template(kind), S.icp_params()
    d2_max = FR.correspondence_threshold(S.BOUND)
    src, near = S.near_and_far(kind)
    _, d2 = O.nn(tpl, src, mode=1)
    assert np.array_equal(d2 <= d2_max, near) and near.sum() == 200 and (~near).sum() == 60
    both, alone = QR.pair(tpl, src, prm, d2_max=d2_max), QR.pair(tpl, src, prm)
    assert both["recip_stats"].last_n0 == 200 and alone["recip_stats"].last_n0 == 260 and both["converged"] and alone["converged"]
    # the variant whose far points are reciprocal: only the bound removes them, and the pose differs (the lattice only: beyond the
    # scanned template's rounded end every far point has one of a few tip points as its neighbour, and one of each is kept)
    if kind != "lattice":
        return
    src, near = S.half_and_far(kind)
    nn, d2 = O.nn(tpl, src, mode=1)
    assert np.array_equal(d2 <= d2_max, near)
    assert IQ.keep_mask(src, tpl, nn, d2)[0][~near].sum() >= 10 and not IQ.keep_mask(src, tpl, nn, d2, d2_max)[0][~near].any()
    both, alone = QR.pair(tpl, src, prm, d2_max=d2_max), QR.pair(tpl, src, prm)
    assert both["kept"][0] < alone["kept"][0] and not np.array_equal(both["T"], alone["T"]) and both["converged"] and not both["stopped"] and not alone["stopped"]


@pytest.mark.parametrize("kind", S.KINDS)
def test_combination_scenarios(kind):
    tpl, prm = S.template(kind), S.icp_params(40)
    src = S.coarse_source(kind)
    fine, st = QR.coarse_pair(tpl, src, prm, S.COARSE)
    single = QR.pair(tpl, src, prm)
    assert st.used == IC.USED and st.n_coarse == 175 and st.coarse_iterations >= 2
    assert not np.array_equal(fine["T"], single["T"]) or fine["iterations"] != single["iterations"]
    far = S.far_source(kind)
    g, flip = cf.guess(cf.shape_frame(far), cf.shape_frame(tpl))
    assert flip >= 0
    guessed = QR.pair(tpl, far, prm, guess=np.asarray(g, f32))
    plain = QR.pair(tpl, far, prm)
    assert guessed["fitness"] < plain["fitness"] and len(set(guessed["kept"])) > 1 and not guessed["stopped"]


def test_fused_scenario_has_both_slots_and_changing_counts():
    case = S.fused_case(-1)
    exp = case.expected()
    clusters = [c for e in exp for c in e["clusters"]]
    assert len(exp) == 3 and len(clusters) >= 12 and all(set(c.pairs) == {0, 1} for c in clusters)      # every cluster against both templates
    assert case.prm.icp_max_iterations == 12
    assert any(len(set(p["kept"])) > 1 for c in clusters for p in c.pairs.values())
    assert any(QR.stats_of(c.pairs[c.slot]).min_kept < c.size for c in clusters)
    off = S.fused_case(-1, False).expected()
    assert any(not np.array_equal(a.T, b.T) for e, o in zip(exp, off) for a, b in zip(e["clusters"], o["clusters"]))
    for slot in (0, 1):
        single = S.fused_case(slot).expected()
        assert all(c.slot == slot for e in single for c in e["clusters"]) and [e["counts"] for e in single] == [e["counts"] for e in exp]
