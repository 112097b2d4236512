"""Rule C19 (median-distance correspondence rejection) without a GPU: the numpy module (perception_amd/icp_reject.py) against a
sort-based restatement, the host arithmetic of icp_reject_math.hpp (icp_reject_math_check, plain and sanitized, and
cd_icp_median_threshold) against the module bit for bit, the reference pair (tests/reject_reference.py) against the oracle's ICP
when nothing is ever rejected, every precondition of the GPU scenarios (tests/reject_scenarios.py) from the reference alone, the
stage planning with the mode on, and the names the header and capi.py export."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fused_reference as FR
import reject_reference as RR
import reject_scenarios as S
from oracle import oracle_py as O
from perception_amd import capi, cluster_frame as cf, icp_coarse as IC, icp_reject as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perception_amd", "csrc")
NEW_SYMBOLS = ["cd_set_icp_median_rejection", "cd_get_icp_median_rejection", "cd_icp_reject_struct_size", "cd_get_cluster_reject_stats",
               "cd_icp_median_threshold"]
f32, f64 = np.float32, np.float64
FACTORS = (0.25, 1.0, 2.5)
HOST_CXX = ["g++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas"]


def test_header_and_capi_export_the_names():
    header = open(os.path.join(ROOT, "include", "cuboid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert re.search(r"#define CD_ABI_VERSION 4\b", header)
    body = re.search(r"typedef struct cd_icp_reject_stats \{(.*?)\} cd_icp_reject_stats;", header, re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[3\])?;", body)
    assert [(t, n, bool(a)) for t, n, a in fields] == [("int32_t", "first_kept", False), ("int32_t", "last_kept", False), ("int32_t", "min_kept", False),
                                                     ("int32_t", "stopped_few", False), ("float", "last_median", False), ("int32_t", "reserved", True)]
    assert [n for n, _ in capi.CdIcpRejectStats._fields_] == [n for _, n, _ in fields]
    assert C.sizeof(capi.CdIcpRejectStats) == 32
    assert "CorrespondenceRejectorMedianDistance" in header and "unpinned" in header
    for fn in (capi.Context.set_icp_median_rejection, capi.Context.icp_median_rejection, capi.Context.cluster_reject_stats, capi.icp_median_threshold):
        assert callable(fn)


def test_library_struct_size_and_host_threshold():
    lib = capi.load_library()
    assert lib.cd_icp_reject_struct_size() == C.sizeof(capi.CdIcpRejectStats)
    for d2, _ in vectors()[::3]:
        for f in FACTORS:
            m, thr = capi.icp_median_threshold(d2, f)
            em, et = IR.threshold(d2, f)
            assert bits32(m) == bits32(em) and bits64(thr) == bits64(et)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.CuboidError):
            capi.icp_median_threshold([1.0, 2.0], bad)
    for bad in ([], [1.0, float("nan")], [1.0, -2.0]):
        with pytest.raises(capi.CuboidError):
            capi.icp_median_threshold(bad, 1.0)


# ---- the module against a sort -------------------------------------------------------------------------------------------------------
def bits32(v):
    return int(np.array([v], f32).view(np.uint32)[0])


def bits64(v):
    return int(np.array([v], f64).view(np.uint64)[0])


def vectors():
    """[(d2 float32, note)]: n = 1 .. 9, 64, 65, 4097 of random squared distances over many exponents, all equal, all zero, one value
    repeated across the median, +inf among them, neighbours in the last bit."""
    rng = np.random.default_rng(5)
    out = []
    for n in list(range(1, 10)) + [64, 65, 4097]:
        out.append(((rng.uniform(0, 1, n) ** 4 * 10.0 ** rng.integers(-8, 1, n)).astype(f32), "random %d" % n))
        out.append((np.full(n, f32(3.25e-5)), "equal %d" % n))
        out.append((np.zeros(n, f32), "zero %d" % n))
        v = (rng.uniform(0, 1e-3, n)).astype(f32)
        v[rng.permutation(n)[:max(1, (2 * n) // 3)]] = np.sort(v)[n // 2]
        out.append((v, "repeated across the median %d" % n))
    v = rng.uniform(0, 1e-3, 65).astype(f32)
    v[::7] = np.inf
    out.append((v, "inf among them"))
    base = np.array([1.0e-4], f32).view(np.uint32)[0]
    out.append(((base + rng.integers(0, 4, 4097).astype(np.uint32)).view(f32), "neighbours in the last bit"))
    out.append((np.full(5, np.inf, f32), "all inf"))
    return out


def by_sort(d2, factor, d2_max=None):
    """Steps 1 - 4 restated with a sort and Python floats (a Python float product is one rounded double product)."""
    d = [float(v) for v in np.asarray(d2, f32)]
    k0 = [i for i, v in enumerate(d) if d2_max is None or v <= float(f32(d2_max))]
    if len(k0) < 3:
        return [i in k0 for i in range(len(d))], None, None, len(k0)
    m = sorted(d[i] for i in k0)[len(k0) // 2]
    thr = m * float(factor)
    return [(i in set(k0)) and d[i] <= thr for i in range(len(d))], m, thr, len(k0)


def test_threshold_and_keep_mask_against_a_sort():
    for d2, note in vectors():
        for f in FACTORS:
            m, thr = IR.threshold(d2, f)
            srt = sorted(float(v) for v in d2)
            assert float(m) == srt[len(d2) // 2] and bits64(thr) == bits64(srt[len(d2) // 2] * f), note
            keep, km, kthr, n0 = IR.keep_mask(d2, f)
            ek, em, et, en0 = by_sort(d2, f)
            assert list(keep) == ek and n0 == en0 == len(d2), note
            if len(d2) >= 3:
                assert float(km) == em and bits64(kthr) == bits64(et), note
                assert keep.sum() >= len(d2) // 2 + 1 if f >= 1.0 else True, note   # (factor >= 1 keeps the median and all below it)
            else:
                assert km is None and kthr is None and keep.all(), note


def test_keep_mask_with_the_bound():
    for d2, note in vectors():
        if len(d2) < 4 or not np.isfinite(d2).all():
            continue
        for q in (0.0, 0.3, 0.8):
            bound = f32(np.quantile(d2.astype(f64), q))
            for f in FACTORS:
                keep, m, thr, n0 = IR.keep_mask(d2, f, d2_max=bound)
                ek, em, et, en0 = by_sort(d2, f, d2_max=bound)
                assert list(keep) == ek and n0 == en0, (note, q)
                assert (m is None) == (em is None) and (m is None or (float(m) == em and bits64(thr) == bits64(et))), (note, q)
    # the rank is taken over the survivors: a bound that removes the upper half moves the median down
    d2 = np.arange(1, 11, dtype=f32)
    assert float(IR.keep_mask(d2, 1.0)[1]) == 6.0 and float(IR.keep_mask(d2, 1.0, d2_max=f32(5.0))[1]) == 3.0
    assert IR.keep_mask(d2, 1.0, d2_max=f32(2.0))[3] == 2 and IR.keep_mask(d2, 1.0, d2_max=f32(2.0))[1] is None
    assert not IR.valid_factor(0.0) and not IR.valid_factor(float("nan")) and not IR.valid_factor(float("inf")) and not IR.valid_factor(-2.0)
    assert IR.valid_factor(0.25)


# ---- the host arithmetic of icp_reject_math.hpp ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["", "-fsanitize=address,undefined"], ids=["plain", "sanitized"])
def check_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_reject") / "icp_reject_math_check")
    subprocess.run(HOST_CXX + ([request.param] if request.param else []) + [os.path.join(CSRC, "icp_reject_math_check.cpp"), "-o", exe], check=True)
    return exe


def test_check_program_equals_the_module_bitwise(check_exe, tmp_path):
    cases = []
    for d2, note in vectors():
        for f in FACTORS:
            cases.append((d2, f, None, note))
        if len(d2) >= 4 and np.isfinite(d2).all():
            cases.append((d2, 2.5, f32(np.quantile(d2.astype(f64), 0.6)), note + " bounded"))
            cases.append((d2, 1.0, f32(0.0), note + " bound 0"))
    for i, (d2, f, bound, note) in enumerate(cases):
        path = str(tmp_path / ("case%d.bin" % i))
        with open(path, "wb") as fp:
            fp.write(struct.pack("<iifid", len(d2), 0 if bound is None else 1, 0.0 if bound is None else float(bound), 0, f) + np.asarray(d2, "<f4").tobytes())
        r = subprocess.run([check_exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (note, r.stdout + r.stderr)
        lines = r.stdout.strip().split("\n")
        keep, m, thr, n0 = IR.keep_mask(d2, f, d2_max=bound)
        assert lines[0].split() == ["counts", str(len(d2)), str(n0), str(int(keep.sum()))], note
        if m is None:
            assert lines[1:3] == ["median none", "thr none"], note
        else:
            assert lines[1] == "median %08x" % bits32(m) and lines[2] == "thr %016x" % bits64(thr), note
        assert lines[3] == "keep " + "".join("1" if k else "0" for k in keep), note
    bad = str(tmp_path / "bad.bin")
    with open(bad, "wb") as fp:
        fp.write(struct.pack("<iifid", 2, 0, 0.0, 0, float("nan")) + np.zeros(2, "<f4").tobytes())
    assert subprocess.run([check_exe, bad], capture_output=True).returncode == 2


def test_pcl_compat_has_the_rejector(tmp_path):
    src = str(tmp_path / "rejector.cpp")
    open(src, "w").write("""#include "pcl_compat.hpp"
namespace pcl = pclhip;
int main() {
    pcl::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
    pcl::registration::CorrespondenceRejectorMedianDistance::Ptr rej(new pcl::registration::CorrespondenceRejectorMedianDistance);
    if (rej->getMedianFactor() != 1.0) return 1;
    rej->setMedianFactor(4.0);
    icp.addCorrespondenceRejector(rej);
    icp.clearCorrespondenceRejectors();
    return rej->getMedianFactor() == 4.0 ? 0 : 1;
}
""")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "perception_amd", "cpp"), src], check=True)


# ---- the stage planning with the mode on -------------------------------------------------------------------------------------------
def test_plan_with_the_mode_on_is_all_sliced(tmp_path):
    exe = str(tmp_path / "icp_plan_check")
    subprocess.run(HOST_CXX + [os.path.join(CSRC, "icp_plan_check.cpp"), "-o", exe], check=True)

    def plan(reject_on, plane_on=0):
        lines = ["n_cu 256", "plane_on %d" % plane_on, "reject_on %d" % reject_on, "slot 0 3 1 0", "slot 1 0 1 0"]
        # 60 clusters of a lattice template and of a gridded one: today the lattice driver and the grouped launch take them all
        lines += ["cluster %d %d 0 1700 0" % (100 + k, k // 8) for k in range(60)] + ["cluster 2 0 0 1700 0"]
        lines += ["cluster %d %d 1700 2979 1" % (700 + k, k // 8) for k in range(60)]
        path = str(tmp_path / ("plan%d%d.txt" % (reject_on, plane_on)))
        open(path, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        return json.loads(r.stdout)
    off, on = plan(0), plan(1)
    assert off["status"] == on["status"] == 0
    assert off["plan"]["reject"] == 0 and off["plan"]["n_lat"] == 60 and (off["plan"]["grouped_pipe"] or off["plan"]["nwork"] == 0 or off["plan"]["whole_cluster"])
    p = on["plan"]
    assert p["reject"] == 1 and p["n_lat"] == 0 and not p["grouped_pipe"] and not p["whole_cluster"] and not p["lat_direct"] and p["icp_search"] == 0
    q = p["qslice"]
    assert p["nwork"] == sum(-(-(100 + k) // q) for k in range(60)) + sum(-(-(700 + k) // q) for k in range(60)) and p["n_live"] == 120
    assert on["tile0"][60] == on["tile0"][61]                        # the cluster of two points has no items
    both = plan(1, plane_on=1)
    assert both["status"] == capi.CD_ERR_INVALID_ARG and "both on" in both["message"]


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


@pytest.mark.parametrize("kind", S.KINDS)
def test_reference_pair_equals_the_oracle_when_nothing_is_rejected(kind):
    tpl, prm = S.template(kind), S.icp_params()
    assert len(tpl) == {"lattice": 1700, "scanned": 2979}[kind]
    for seed in (2, 3):
        src, _ = RR.contamination_scene(tpl, seed)
        for guess in (None, np.array(cf.guess(cf.shape_frame(src), cf.shape_frame(tpl))[0], f32)):
            e = RR.pair(tpl, src, prm, 1.0e30, guess=guess)
            r, al = oracle_pair(tpl, src, prm, guess)
            assert e["T"].view(np.uint32).ravel().tolist() == np.array(list(r.T), f32).view(np.uint32).tolist()
            assert (e["iterations"], e["converged"], e["accepted"]) == (r.iterations, r.converged, r.accepted) and bits64(e["fitness"]) == bits64(r.fitness)
            assert np.array_equal(e["aligned"].view(np.uint32), al.view(np.uint32))
            assert e["reject_stats"][:4] == (len(src), len(src), len(src), 0) and e["iterations"] > 3


# ---- the preconditions of the GPU scenarios -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_contamination_scene_is_helped_by_the_rule(kind):
    tpl, prm = S.template(kind), S.icp_params()
    for seed in S.SCENE_SEEDS:
        src, truth = RR.contamination_scene(tpl, seed)
        assert len(src) == 1800
        r, _ = oracle_pair(tpl, src, prm)
        on = RR.pair(tpl, src, prm, S.FACTOR)
        err_off = RR.translation_error(np.array(list(r.T)).reshape(4, 4), truth)
        err_on = RR.translation_error(on["T"], truth)
        assert err_on < err_off, (kind, seed, err_on, err_off)
        assert on["converged"] and len(set(on["kept"])) > 1 and on["reject_stats"].min_kept < 1800      # the kept counts change over the iterations
    assert set(S.GPU_SCENE_SEEDS) <= set(S.SCENE_SEEDS)


@pytest.mark.parametrize("kind", S.KINDS)
def test_sized_sources_cover_the_paths(kind):
    tpl, prm = S.template(kind), S.icp_params()
    assert {3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} <= set(S.SIZES) and max(S.SIZES) > 4096
    varied = 0
    for n in S.SIZES:
        e = RR.pair(tpl, S.sized_source(kind, n, n), prm, S.FACTOR)
        assert e["converged"] and not e["stopped"] and e["iterations"] >= 2, n
        assert e["reject_stats"].first_kept >= n // 2 + 1
        if n >= 63:
            assert e["reject_stats"].min_kept < n, n       # something is rejected
        varied += len(set(e["kept"])) > 1
    assert varied >= 6


def test_tie_sources_are_ties():
    prm = S.icp_params()
    for kind in S.KINDS:
        tpl = S.template(kind)
        src = S.exact_subset(kind)
        _, d2 = O.nn(tpl, src, mode=1)
        assert (d2 == 0).all()
        e = RR.pair(tpl, src, prm, S.FACTOR)
        assert e["kept"] == [len(src)] and e["iterations"] == 1 and e["converged"] and e["reject_stats"].last_median_bits == 0
        assert np.abs(e["T"] - np.eye(4, dtype=f32)).max() < 1e-6     # (the float32 SVD of a perfect match: the identity to rounding)
    tpl = S.template("lattice")
    src = S.shifted_face()
    _, d2 = O.nn(tpl, src, mode=1)
    assert len(set(d2.view(np.uint32).tolist())) == 1 and d2[0] > 0
    e = RR.pair(tpl, src, prm, S.FACTOR)
    assert e["kept"][0] == len(src) and e["converged"]
    src = S.half_at_the_median()
    _, d2 = O.nn(tpl, src, mode=1)
    m, thr = IR.threshold(d2, S.FACTOR)
    assert (d2 == m).sum() >= len(src) // 2 and (d2 < m).sum() > 0 and (d2.astype(f64) > thr).sum() == len(src) // 6
    assert np.sort(d2)[len(src) // 2 - 1] == m == np.sort(d2)[len(src) // 2 + 1]      # the value repeats across the median rank
    e = RR.pair(tpl, src, prm, S.FACTOR)
    assert e["kept"][0] == len(src) - len(src) // 6 and e["converged"]


@pytest.mark.parametrize("kind", S.KINDS)
def test_stop_scenarios_stop(kind):
    tpl, prm = S.template(kind), S.icp_params()
    src = S.stops_at_once(kind)
    e = RR.pair(tpl, src, prm, S.SMALL_FACTOR)
    assert len(src) == 6 and e["kept"] == [2] and (e["iterations"], e["converged"], e["accepted"], e["stopped"]) == (0, 0, 0, 1)
    assert np.array_equal(e["T"], np.eye(4, dtype=f32)) and np.array_equal(e["aligned"], src) and e["reject_stats"].stopped_few == 1
    later = RR.pair(tpl, S.stops_later(kind), prm, S.SMALL_FACTOR)
    assert later["stopped"] and later["iterations"] >= 2 and not later["converged"] and later["kept"][-1] < 3 and min(later["kept"][:-1]) >= 3
    assert not np.array_equal(later["T"], np.eye(4, dtype=f32))                         # Tfinal as it stood at the stop


@pytest.mark.parametrize("kind", S.KINDS)
def test_bound_scenario_rejects_exactly_the_far_points(kind):
    tpl, prm = S.template(kind), S.icp_params()
    src, near = S.near_and_far(kind)
    d2_max = FR.correspondence_threshold(S.BOUND)
    _, d2 = O.nn(tpl, src, mode=1)
    assert np.array_equal(d2 <= d2_max, near) and near.sum() == 200 and (~near).sum() == 60
    both = RR.pair(tpl, src, prm, S.FACTOR, d2_max=d2_max)
    alone = RR.pair(tpl, src, prm, S.FACTOR)
    m_both, m_alone = IR.keep_mask(d2, S.FACTOR, d2_max=d2_max)[1], IR.keep_mask(d2, S.FACTOR)[1]
    assert m_both == np.sort(d2[near])[100] < m_alone == np.sort(d2)[130]               # the rank is taken over the survivors
    assert both["kept"][0] <= 200 and both["kept"] != alone["kept"]
    assert both["reject_stats"].last_median_bits != alone["reject_stats"].last_median_bits
    assert not np.array_equal(both["T"], alone["T"]) and both["converged"] and alone["converged"]


@pytest.mark.parametrize("kind", S.KINDS)
def test_combination_scenarios(kind):
    tpl, prm = S.template(kind), S.icp_params(40)
    src = S.coarse_source(kind)
    fine, st = RR.coarse_pair(tpl, src, prm, S.FACTOR, S.COARSE)
    single = RR.pair(tpl, src, prm, S.FACTOR)
    assert st.used == IC.USED and st.n_coarse == 175 and st.coarse_iterations >= 2
    assert not np.array_equal(fine["T"], single["T"]) or fine["iterations"] != single["iterations"]
    far = S.far_source(kind)
    g, flip = cf.guess(cf.shape_frame(far), cf.shape_frame(tpl))
    assert flip >= 0
    assert RR.coarse_pair(tpl, far, prm, S.FACTOR, (4, 64), guess_mode="cluster")[1].used == IC.USED
    guessed = RR.pair(tpl, far, prm, S.FACTOR, guess=np.asarray(g, f32))
    plain = RR.pair(tpl, far, prm, S.FACTOR)
    assert guessed["fitness"] < plain["fitness"] and len(set(guessed["kept"])) > 1


def test_fused_scenario_has_both_slots_and_changing_counts():
    case = S.fused_case(-1)
    exp = case.expected()
    clusters = [c for e in exp for c in e["clusters"]]
    assert len(exp) == 3 and len(clusters) >= 12 and {c.slot for c in clusters} == {0, 1}
    assert any(len(set(p["kept"])) > 1 for c in clusters for p in c.pairs.values())
    assert all(RR.stats_of(c).first_kept >= c.size // 2 + 1 for c in clusters)
    off = S.fused_case(-1, 0).expected()
    assert any(not np.array_equal(a.T, b.T) for e, o in zip(exp, off) for a, b in zip(e["clusters"], o["clusters"]))
    single = S.fused_case(1).expected()
    assert all(c.slot == 1 for e in single for c in e["clusters"]) and [e["counts"] for e in single] == [e["counts"] for e in exp]
