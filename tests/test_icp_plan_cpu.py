"""ICP stage planning on the CPU (no GPU): perception_amd/csrc/icp_plan.hpp through its stand-alone program icp_plan_check.
Every case below describes one ICP stage (clusters, template slots, tunables, calls in flight); the program prints every decision
of the planner and of the launch sizing as JSON.

Two checks.  (1) The output equals icp_plan_expected.json, recorded when the planning code had just been moved out of
cuboid_hip.hip, text unchanged.  The file is data (long lists packed by pack() below, nothing lost): an entry that differs means
a batch now takes another driver or another launch shape - the numeric results would not show it, the drivers agree bit for bit.  (2) The table alone compares the code with itself,
so the edges of every rule the planner's comments state are asserted here directly."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "perception_amd", "csrc")
EXE = os.path.join(CSRC, "icp_plan_check")
with open(os.path.join(ROOT, "tests", "icp_plan_expected.json")) as _f:
    EXPECTED = json.load(_f)

N_CU = 256                      # MI355X
ICP_TPL_LDS, ICP_QSLICE, CD_PIPE_SLOTS = 7552, 512, 4      # common.hpp
OK, INVALID_ARG, CAPACITY, FEW, NO_TEMPLATE = 0, -1, -2, -5, -7      # cuboid_hip.h
GUESS_PARAMS, GUESS_PER_FRAME, GUESS_SURFACE, GUESS_CLUSTER = 1, 2, 3, 4
IDENTITY = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]

# template slots by kind: (faces, gridded, big) and a point count on the right side of ICP_TPL_LDS
LDS = {"flags": (0, 1, 0), "m": 5000}          # kind 1: k_icp_pipe
LDS_EDGE = {"flags": (0, 1, 0), "m": ICP_TPL_LDS}
BIG = {"flags": (0, 1, 1), "m": ICP_TPL_LDS + 1}   # kind 2: k_icp_pipe_big
NOPIPE = {"flags": (0, 0, 0), "m": 5000}       # kind 0: not gridded
BIG_NOT_OK = {"flags": (0, 1, 0), "m": 9000}   # kind 0: too large for LDS, nothing for k_icp_pipe_big
LATTICE = {"flags": (3, 1, 0), "m": 5000}
EMPTY = {"flags": (0, 0, 0), "m": 0}


def stage(slots, clusters, tun=None, queries=(), done=(), **scalars):
    """slots: one template description per slot; clusters: (n, frame, slot), in order -> the text of a case"""
    lines = ["%s %d" % kv for kv in sorted(scalars.items())]
    for name, val in sorted((tun or {}).items()):
        lines.append("tun %s %s" % (name, " ".join(str(v) for v in val) if isinstance(val, tuple) else val))
    for s, t in enumerate(slots):
        lines.append("slot %d %d %d %d" % ((s,) + t["flags"]))
    for n, frame, slot in clusters:
        lines.append("cluster %d %d %d %d %d" % (n, frame, 10000 * slot, slots[slot]["m"], slot))
    lines += ["done %d %d" % d for d in done]
    lines += list(queries)
    return "\n".join(lines) + "\n"


def same(n_clusters, slot=0, n=100):
    return [(n, k // 4, slot) for k in range(n_clusters)]


def sizes(ns, slot=0):
    return [(n, k, slot) for k, n in enumerate(ns)]


MIXED5 = [LDS, BIG, LDS, BIG, LDS]      # kinds 1 2 1 2 1
MIXED5_CLUSTERS = (sizes([300, 900, 2, 500], 0) + sizes([4000, 100], 1) + sizes([50] * 7, 2) + sizes([2500, 2600, 2400], 3) +
                   sizes([10, 20, 30, 40, 50, 60, 70, 80, 90], 4))
GROUPED_CASES = {
    "grouped_mixed5": dict(tun={"icp_mode": 3}),
    "grouped_mixed5_wg8": dict(tun={"icp_mode": 3, "icp_max_wg": 8}),
    "grouped_mixed5_wg5": dict(tun={"icp_mode": 3, "icp_max_wg": 5}),
    "grouped_mixed5_wg26": dict(tun={"icp_mode": 3, "icp_max_wg": 26}),
    "grouped_mixed5_wg25": dict(tun={"icp_mode": 3, "icp_max_wg": 25}),
    "grouped_mixed5_weight7": dict(tun={"icp_mode": 3, "icp_big_weight": 7}),
    "grouped_mixed5_cpw3": dict(tun={"icp_mode": 3, "icp_cpw": 3}),
    "grouped_mixed5_slots3": dict(tun={"icp_mode": 3, "icp_slots": 3}, batches_in_flight=5),
    "grouped_mixed5_crowded": dict(tun={"icp_mode": 3}, batches_in_flight=5),
}
LAT_DIRECT_OFF = ("icp_direct", "mirror_reads", "mirror_writes", "copy_kernels")
GUESS_MODES = {"params": GUESS_PARAMS, "per_frame": GUESS_PER_FRAME, "surface": GUESS_SURFACE, "cluster": GUESS_CLUSTER}

CASES = {
    # driver choice in auto mode
    "mode_cluster": stage([LDS], same(5), tun={"icp_mode": 2}),
    "mode_pipe_two_groups": stage([NOPIPE, LDS], same(1, 0) + same(1, 1), tun={"icp_mode": 3}),
    "mode_pipe_one_group": stage([LDS], same(3), tun={"icp_mode": 3}),
    "mode_pipe_no_live_pipe_cluster": stage([NOPIPE, LDS], same(4, 0) + same(1, 1, n=2), tun={"icp_mode": 3}),
    # grouped
    "grouped_ncu8_two": stage([LDS, BIG], same(1, 0) + same(1, 1), n_cu=8),
    "grouped_ncu8_one": stage([LDS, BIG], same(1, 0) + same(1, 1, n=2), n_cu=8),
    "grouped_16_groups": stage([LDS, BIG], [(100, g, g % 2) for g in range(16)], tun={"icp_mode": 3}),
    "grouped_17_groups": stage([LDS, BIG], [(100, g, g % 2) for g in range(17)], tun={"icp_mode": 3}),
    "grouped_no_pipe_kind": stage([NOPIPE, BIG_NOT_OK], same(3, 0) + same(3, 1), tun={"icp_mode": 3}),
    # lattice
    "lat_all": stage([LATTICE], sizes([500, 100, 900, 100, 3])),
    "lat_all_premarked": stage([LATTICE, EMPTY], sizes([500, 2, 900]) + sizes([70], 1)),
    "lat_mixed": stage([LATTICE, LDS], sizes([500, 100, 900], 0) + sizes([1200], 1)),
    "lat_off": stage([LATTICE], sizes([500, 100, 900]), tun={"icp_lattice": 0}),
    "lat_shape_override": stage([LATTICE], same(20), tun={"lat_shape": (2, 4, 3)}),
    # rule C17
    "plane_mode_sliced": stage([LATTICE], same(4), plane_on=1, tun={"icp_mode": 1, "icp_lattice": 0}),
    "plane_not_a_lattice": stage([LATTICE, LDS], same(4, 0) + same(1, 1), plane_on=1),
    "plane_not_a_lattice_dead": stage([LATTICE, LDS], same(4, 0) + same(1, 1, n=2), plane_on=1),
    # pre-marked clusters
    "premarked": stage([LDS, EMPTY], sizes([2, 3, 100], 0) + sizes([100], 1) + sizes([700], 0)),
    # work list
    "work_tiny": stage([LDS], sizes([3, 64, 65, 129])),
    "work_cap_reached": stage([LDS], sizes([3, 64, 65, 129]), work_cap=7),
    "work_cap_exceeded": stage([LDS], sizes([3, 64, 65, 129]), work_cap=6),
    # guesses
    "guess_per_frame_short": stage([LDS], [(100, 0, 0), (100, 3, 0), (100, 1, 0)], use_guess=GUESS_PER_FRAME, guess_frames=3),
    # the other drivers' sizing
    "persist_8": stage([LDS], sizes([100, 2, 100, 100, 100, 100, 100, 100])),
    "persist_9": stage([LDS], sizes([100] * 9)),
    "persist_off": stage([LDS], sizes([100] * 3), tun={"icp_persist": 0}),
    "persist_siblings": stage([LDS], sizes([100] * 3), calls_in_flight=2),
    "persist_siblings_forced": stage([LDS], sizes([100] * 3), tun={"icp_persist": 2}, calls_in_flight=2),
    "persist_nwork_G": stage([LDS], sizes([64, 128, 192]), tun={"icp_max_wg": 6}),
    "persist_nwork_G_plus_1": stage([LDS], sizes([64, 128, 192]), tun={"icp_max_wg": 5}),
    "persist_no_work": stage([LATTICE], sizes([100] * 3)),
    "repack": stage([LDS], sizes([200, 64, 2, 130, 100]), done=[(1, 0), (3, 1), (4, 0), (4, 1)]),
    "repack_all_done": stage([LDS], sizes([200, 2, 64]), done=[(0, 0), (0, 1), (2, 0), (2, 1)]),
    "repack_one_slot_open": stage([LDS], sizes([200, 2, 64]), done=[(0, 0), (0, 1), (2, 0)]),
}
CASES.update({name: stage(MIXED5, MIXED5_CLUSTERS, **kw) for name, kw in GROUPED_CASES.items()})
CASES.update({"lat_all_%s_0" % t: stage([LATTICE], sizes([500, 100, 900]), tun={t: 0}) for t in LAT_DIRECT_OFF})
for _name, _mode in GUESS_MODES.items():
    CASES["lat_all_guess_" + _name] = stage([LATTICE], sizes([500, 100, 900]), use_guess=_mode, guess_frames=3)
    CASES["guess_" + _name] = stage([LDS, EMPTY], [(100, 0, 0), (2, 3, 0), (300, 1, 0), (50, 2, 1)], use_guess=_mode, guess_frames=4)

LAT_QUERIES = [(95, 100, 1), (96, 100, 1), (767, 100, 1), (768, 100, 1), (2000, 4096, 1), (2000, 4097, 1), (2000, 16384, 1), (2000, 16385, 1),
               (50, 4097, 1), (256, 8192, 3), (255, 8192, 3), (256, 8193, 3), (256, 8192, 2), (1, 10, 1), (0, 0, 1)]
GRID_QUERIES = [(n, cap, cpw, crowded, slots) for n in (1, 31, 100, 256, 257, 522, 1000, 5000) for cap in (8, 100, 256)
                for cpw, crowded, slots in ((0, 0, 2), (0, 1, 4), (0, 1, 2), (3, 1, 4))]
DONATE_QUERIES = [(d, b, ncl, grid) for d in (-1, 0, 1) for b in (0, 1, 2) for ncl, grid in ((256, 256), (257, 256))]
SLOTS_QUERIES = [(s, b, g) for s in (0, 1, 3, 4, 9) for b in (1, 3, 4, 7) for g in (0, 1)]
CASES["queries"] = stage([], [], queries=["lat %d %d %d" % q for q in LAT_QUERIES] + ["grid %d %d %d %d %d" % q for q in GRID_QUERIES] +
                         ["donate %d %d %d %d" % q for q in DONATE_QUERIES] + ["slots %d %d %d" % q for q in SLOTS_QUERIES])
CASES["queries_lat_shape"] = stage([], [], tun={"lat_shape": (8, 2, 0)}, queries=["lat %d %d %d" % q for q in LAT_QUERIES])

# Not part of the table, asserted below only: the stages of more than 50 clusters (their output is long, and what the table would
# add to the assertions is small) and the decisions that had no function of their own when the table was recorded
PLANE_GRID_QUERIES = [(no, cap) for no in (0, 1, 511, 512, 513, 5000) for cap in (1, 8, 256)]
UNRECORDED = {
    "auto_51": stage([LDS], same(51)),
    "auto_52": stage([LDS], same(52)),
    "auto_52_lds_edge": stage([LDS_EDGE], same(52)),
    "auto_52_big": stage([BIG], same(52)),
    "auto_52_nopipe": stage([BIG_NOT_OK], same(52)),
    "auto_52_two_templates": stage([LDS, LDS], same(26, 0) + same(26, 1)),
    "grouped_auto_mixed": stage([LDS, NOPIPE, BIG], same(40, 0) + same(10, 1) + same(20, 2)),
    "plane_all": stage([LATTICE, LATTICE], same(30, 0) + same(30, 1), plane_on=1),
    "whole_donate_always": stage([LDS], same(60), tun={"icp_donate": 1}, batches_in_flight=6),
    "auto_600_two_templates": stage([LDS, NOPIPE], same(300, 0) + same(300, 1)),
    "mode_sliced": stage([LDS, LATTICE], same(60, 0) + same(60, 1), tun={"icp_mode": 1}),
    "grouped_many_rows": stage([LDS, LDS], same(520, 0) + same(520, 1), tun={"icp_mode": 3, "icp_max_wg": 2000}, n_cu=2000),
    "lat_busy_256": stage([LATTICE], same(256), batches_in_flight=3),
    "work_middle": stage([LDS], sizes([10000] * 10)),
    "work_large": stage([LDS], sizes([9000] * 30)),
    "whole_crowded_522": stage([LDS], same(522), batches_in_flight=4),
    "whole_alone_522": stage([LDS], same(522)),
    "whole_two_in_flight_522": stage([LDS], same(522), batches_in_flight=2),
    "whole_cpw": stage([LDS], same(522), tun={"icp_cpw": 3}),
    "whole_donate_never": stage([LDS], same(522), tun={"icp_donate": 0}),
    "queries_unrecorded": stage([], [], queries=["planegrid %d %d" % q for q in PLANE_GRID_QUERIES] + ["pollgroup %d" % n for n in range(4)]),
}
ALL_CASES = dict(CASES, **UNRECORDED)


def pack(x):
    """lists of more than 8 elements as runs [element, count] - of the differences, when every element is an integer - where
    that is shorter"""
    if isinstance(x, dict):
        return {k: pack(v) for k, v in x.items()}
    if not isinstance(x, list):
        return x
    if len(x) <= 8:
        return [pack(v) for v in x]
    ints = all(type(v) is int for v in x)
    seq = [b - a for a, b in zip([0] + x, x)] if ints else x
    runs = []
    for v in seq:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    packed = {"steps" if ints else "runs": [[pack(v), n] for v, n in runs]}
    return packed if len(runs) * 2 < len(x) else [pack(v) for v in x]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """every case through the program, once"""
    subprocess.run(["make", "-C", CSRC, "icp_plan_check"], check=True, stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("icp_plan")
    res = {}
    for name, text in ALL_CASES.items():
        path = os.path.join(str(d), name + ".txt")
        with open(path, "w") as f:
            f.write(text)
        r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stderr)
        res[name] = json.loads(r.stdout)
    return res


def test_every_case_has_a_recorded_output():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_decisions_are_the_recorded_ones(out, name):
    assert pack(out[name]) == EXPECTED[name]


def plan(out, name):
    assert out[name]["status"] == OK, out[name]
    return out[name]["plan"]


def states(o):
    """the initial states of every cluster: status and done of both parity slots, whether the slots are equal byte for byte,
    whether prev_mse is DBL_MAX, Tfinal of slot 0"""
    return [{"status": s[0:2], "done": s[2:4], "same": s[4], "prev_mse_max": s[5], "Tfinal": s[6] or IDENTITY} for s in o["states"]]


# ---- driver choice in auto mode ----------------------------------------------------------------------------------------------
def test_whole_cluster_from_a_fifth_of_the_cus(out):
    assert 51 * 5 < N_CU <= 52 * 5
    assert not plan(out, "auto_51")["whole_cluster"]
    for name, pipe_ok, big_ok in (("auto_52", 1, 0), ("auto_52_lds_edge", 1, 0), ("auto_52_big", 0, 1)):
        p = plan(out, name)
        assert (p["whole_cluster"], p["pipe_ok"], p["big_ok"], p["grouped_pipe"]) == (1, pipe_ok, big_ok, 0), name
    p = plan(out, "auto_52_nopipe")     # (a template no pipelined kernel takes: sliced in auto mode)
    assert (p["whole_cluster"], p["pipe_ok"], p["big_ok"]) == (0, 0, 0)


def test_two_templates_are_never_whole_cluster_in_auto_mode(out):
    for name in ("auto_52_two_templates", "auto_600_two_templates", "grouped_auto_mixed"):
        p = plan(out, name)
        assert not p["whole_cluster"] and not p["pipe_ok"] and not p["big_ok"], name


def test_forced_modes(out):
    p = plan(out, "mode_cluster")
    assert (p["whole_cluster"], p["pipe_ok"], p["big_ok"]) == (1, 0, 0)
    p = plan(out, "mode_sliced")
    assert (p["grouped_pipe"], p["whole_cluster"], p["n_lat"]) == (0, 0, 0) and not any(p["in_lat"])
    assert p["nwork"] > 0 and p["icp_search"] == 0
    assert plan(out, "mode_pipe_two_groups")["grouped_pipe"] == 1
    p = plan(out, "mode_pipe_one_group")            # one group: nothing to group, the whole-cluster launch takes it
    assert (p["grouped_pipe"], p["whole_cluster"]) == (0, 1)
    assert plan(out, "mode_pipe_no_live_pipe_cluster")["grouped_pipe"] == 0


# ---- grouped -----------------------------------------------------------------------------------------------------------------
def test_grouped_thresholds(out):
    p = plan(out, "grouped_ncu8_two")
    assert [g[3] for g in p["groups"]] == [1, 2] and p["grouped_pipe"] == 1      # n_grouped = 2: 2 * 5 >= 8
    assert plan(out, "grouped_ncu8_one")["grouped_pipe"] == 0                        # n_grouped = 1: 5 < 8
    assert len(plan(out, "grouped_16_groups")["groups"]) == 16 and plan(out, "grouped_16_groups")["grouped_pipe"] == 1
    assert len(plan(out, "grouped_17_groups")["groups"]) == 17 and plan(out, "grouped_17_groups")["grouped_pipe"] == 0
    p = plan(out, "grouped_no_pipe_kind")
    assert [g[3] for g in p["groups"]] == [0, 0] and p["grouped_pipe"] == 0
    p = plan(out, "grouped_auto_mixed")     # 60 clusters in pipe groups: 300 >= 256; the kind-0 group stays sliced
    assert p["grouped_pipe"] == 1 and {w[0] for w in out["grouped_auto_mixed"]["work"]} == set(range(40, 50))


@pytest.mark.parametrize("name", sorted(GROUPED_CASES) + ["grouped_16_groups", "grouped_auto_mixed", "grouped_ncu8_two", "grouped_many_rows"])
def test_grouped_launch_table(out, name):
    o, p = out[name], plan(out, name)
    g, wg_cap = o["grouped"], p["wg_cap"]
    tun = dict(GROUPED_CASES.get(name, {}).get("tun", {}))
    cpw = max(1, tun.get("icp_cpw", 0))
    live = [grp for grp in p["groups"] if grp[3] and grp[2] > 0]      # [beg, end, live, kind, pts]
    live_all = sum(grp[2] for grp in p["groups"] if grp[3])
    assert g["big_weight"] == (tun["icp_big_weight"] if "icp_big_weight" in tun else (4 if live_all <= wg_cap else 2))
    # queues are numbered in launch order: every kind-1 group, then every kind-2 group
    queued = sorted(live, key=lambda grp: grp[3])
    assert [grp[3] for grp in queued] == sorted(grp[3] for grp in live)
    assert len(g["share"]) == len(queued)
    for grp, share in zip(queued, g["share"]):
        assert 1 <= share <= max(1, -(-grp[2] // cpw)), (grp, share)
    if len(queued) <= wg_cap:
        assert sum(g["share"]) <= wg_cap
    assert g["n_wg"] == sum(g["share"]) == g["wg_of"][1] + g["wg_of"][2]
    assert g["wg_of"][1] == sum(s for grp, s in zip(queued, g["share"]) if grp[3] == 1)
    # the order array: group after group, each its clusters with n >= 3, largest first, ties in cluster order
    n_of = [int(line.split()[1]) for line in ALL_CASES[name].splitlines() if line.startswith("cluster ")]
    expect_order, ranges = [], []
    for grp in queued:
        ks = sorted((k for k in range(grp[0], grp[1]) if n_of[k] >= 3), key=lambda k: -n_of[k])
        ranges.append((len(expect_order), len(expect_order) + len(ks)))
        expect_order += ks
    assert g["order"] == expect_order
    # the table: share[q] rows (begin, end, q) per queue, in queue order, 1024 rows at the most
    rows = [tuple(g["tab"][i:i + 3]) for i in range(0, len(g["tab"]), 3)]
    expect_rows = [(b, e, q) for q, ((b, e), share) in enumerate(zip(ranges, g["share"])) for _ in range(share)]
    assert rows == expect_rows[:1024]
    assert g["tab_of"][1] == 0 and g["tab_of"][2] == 3 * min(g["wg_of"][1], 1024)
    assert all(rows[i][2] <= rows[i + 1][2] for i in range(len(rows) - 1))
    n_kind1 = sum(1 for grp in queued if grp[3] == 1)
    assert all((q < n_kind1) == (i < g["wg_of"][1]) for i, (_, _, q) in enumerate(rows))
    assert g["slots"] == (min(tun["icp_slots"], CD_PIPE_SLOTS) if tun.get("icp_slots", 0) > 0 else 2)


def test_grouped_table_is_capped_at_1024_rows(out):
    g = out["grouped_many_rows"]["grouped"]
    assert g["n_wg"] > 1024 and len(g["tab"]) == 3 * 1024


# ---- lattice -----------------------------------------------------------------------------------------------------------------
def test_lattice_stage(out):
    p = plan(out, "lat_all")
    assert p["n_lat"] == p["n_live"] == 5 and p["icp_search"] == 1 and p["nwork"] == 0 and p["lat_direct"] == 1
    assert out["lat_all"]["lat"]["order"] == [2, 0, 1, 3, 4]       # largest first, ties in cluster order
    p = plan(out, "lat_all_premarked")                            # pre-marked clusters do not count
    assert (p["n_lat"], p["n_live"], p["lat_direct"], p["in_lat"]) == (2, 2, 1, [1, 0, 1, 0])
    p = plan(out, "lat_mixed")
    assert (p["n_lat"], p["n_live"], p["icp_search"], p["lat_direct"]) == (3, 4, 2, 0)
    assert out["lat_mixed"]["work"] and {w[0] for w in out["lat_mixed"]["work"]} == {3}
    p = plan(out, "lat_off")
    assert (p["n_lat"], p["icp_search"], p["lat_direct"]) == (0, 0, 0) and p["nwork"] > 0


@pytest.mark.parametrize("name", ["lat_all_%s_0" % t for t in LAT_DIRECT_OFF] + ["lat_all_guess_" + g for g in sorted(GUESS_MODES)])
def test_lat_direct_needs_every_mirror_and_no_guess(out, name):
    p = plan(out, name)
    assert p["n_lat"] == p["n_live"] == 3 and p["icp_search"] == 1 and p["lat_direct"] == 0


# ---- rule C17 ----------------------------------------------------------------------------------------------------------------
def test_plane_weighted_stage(out):
    for name in ("plane_all", "plane_mode_sliced"):
        p = plan(out, name)
        assert (p["plane"], p["nwork"], p["grouped_pipe"], p["n_lat"], p["icp_search"], p["lat_direct"]) == (1, 0, 0, 0, 1, 0), name
    assert out["plane_not_a_lattice"]["status"] == INVALID_ARG
    assert out["plane_not_a_lattice"]["message"] == "plane-weighted ICP is on and a template of the call is not a lattice"
    assert plan(out, "plane_not_a_lattice_dead")["plane"] == 1      # (a cluster that is not live asks nothing of its template)


# ---- pre-marked clusters -----------------------------------------------------------------------------------------------------
def test_premarked_clusters(out):
    o, p = out["premarked"], plan(out, "premarked")
    st = states(o)
    assert st[0]["status"] == [FEW, FEW] and st[0]["done"] == [1, 1]
    assert st[3]["status"] == [NO_TEMPLATE, NO_TEMPLATE] and st[3]["done"] == [1, 1]
    for k in (1, 2, 4):
        assert st[k]["status"] == [OK, OK] and st[k]["done"] == [0, 0]
    assert p["n_live"] == 3
    assert {w[0] for w in o["work"]} == {1, 2, 4}           # n = 3 is live; the pre-marked ones get no tiles
    assert all(s["same"] == 1 and s["prev_mse_max"] == 1 and s["Tfinal"] == IDENTITY for s in st)


# ---- work list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["work_tiny", "work_middle", "work_large", "premarked", "lat_mixed", "grouped_auto_mixed", "repack"])
def test_work_list(out, name):
    o, p = out[name], plan(out, name)
    q = p["qslice"]
    assert 64 <= q <= ICP_QSLICE and q % 16 == 0
    tiles = [0] * p["ncl"]
    for k, t in o["work"]:
        assert t == tiles[k]                                 # a cluster's tiles in order
        tiles[k] += 1
    assert [w[0] for w in o["work"]] == sorted(w[0] for w in o["work"])
    assert o["tile0"] == [sum(tiles[:k]) for k in range(p["ncl"])] and p["nwork"] == sum(tiles) == len(o["work"])
    n_of = [int(line.split()[1]) for line in ALL_CASES[name].splitlines() if line.startswith("cluster ")]
    assert all(t in (0, -(-n // q)) for t, n in zip(tiles, n_of))


def test_qslice(out):
    assert plan(out, "work_tiny")["qslice"] == 64
    assert plan(out, "work_large")["qslice"] == ICP_QSLICE       # 270 000 points: 527 slices of 512
    assert plan(out, "work_middle")["qslice"] == 208              # 100 000 points / 512 = 195, rounded up to 16s
    assert [w[0] for w in out["work_tiny"]["work"]] == [0, 1, 2, 2, 3, 3, 3]


def test_work_capacity(out):
    assert plan(out, "work_cap_reached")["nwork"] == 7
    assert out["work_cap_exceeded"]["status"] == CAPACITY and out["work_cap_exceeded"]["message"] == "ICP work list overflow"


# ---- guesses -----------------------------------------------------------------------------------------------------------------
def test_guesses(out):
    short = out["guess_per_frame_short"]       # frames 0 .. 3 need four matrices
    assert short["status"] == INVALID_ARG
    assert short["message"] == "icp_use_guess = CD_GUESS_PER_FRAME but cd_set_frame_guesses holds fewer frames than the batch"
    frame_of = [0, 3, 1, 2]
    per_frame = [[1000.0 * f + i for i in range(16)] for f in frame_of]
    single = [-(i + 1.0) for i in range(16)]
    for name, mode, need, tfinal in (("params", GUESS_PARAMS, 16, [single] * 4), ("per_frame", GUESS_PER_FRAME, 64, per_frame),
                                     ("surface", GUESS_PER_FRAME, 64, per_frame), ("cluster", GUESS_CLUSTER, 64, [IDENTITY] * 4)):
        o, p = out["guess_" + name], plan(out, "guess_" + name)
        assert (p["guess_mode"], p["guess_need"], p["max_n"]) == (mode, need, 300), name
        st = states(o)
        assert [s["Tfinal"] for s in st] == tfinal, name
        assert all(s["same"] == 1 for s in st)
        assert st[1]["status"] == [FEW, FEW] and st[3]["status"] == [NO_TEMPLATE, NO_TEMPLATE]
    assert plan(out, "auto_52")["guess_need"] == 0 and plan(out, "auto_52")["guess_mode"] == 0


# ---- lat_launch_shape --------------------------------------------------------------------------------------------------------
def test_lat_launch_shape(out):
    got = dict(zip(LAT_QUERIES, out["queries"]["queries"]))
    wpc = {q: s[1] for q, s in got.items()}
    assert (wpc[(95, 100, 1)], wpc[(96, 100, 1)], wpc[(767, 100, 1)], wpc[(768, 100, 1)]) == (16, 8, 8, 4)
    assert wpc[(2000, 4096, 1)] == 4 and wpc[(2000, 4097, 1)] == 8 and wpc[(2000, 16384, 1)] == 8 and wpc[(2000, 16385, 1)] == 16
    assert wpc[(50, 4097, 1)] == 16                       # "at least 8": fewer clusters keep their 16
    assert got[(256, 8192, 3)][:3] == [4, 2, 1]
    for q in ((255, 8192, 3), (256, 8193, 3), (256, 8192, 2)):
        assert got[q][:2] != [4, 2] and got[q][0] == 1, q
    for (n_lat, _, _), (cpw, _, per_slot, n_wg) in got.items():
        assert n_wg == max(1, -(-n_lat // (cpw * per_slot)))
    forced = dict(zip(LAT_QUERIES, out["queries_lat_shape"]["queries"]))
    for (n_lat, _, _), s in forced.items():
        assert s == [8, 2, 1, max(1, -(-n_lat // 8))]      # (clusters per slot: at least 1)
    assert out["lat_shape_override"]["lat"] == {"cpw": 2, "wpc": 4, "per_slot": 3, "n_wg": 4, "order": list(range(20))}
    lat = out["lat_busy_256"]["lat"]
    assert (lat["cpw"], lat["wpc"], lat["n_wg"]) == (4, 2, 64)


# ---- whole_launch_grid, whole_donate, pipe_slots -----------------------------------------------------------------------------
def test_whole_launch_grid(out):
    base = len(LAT_QUERIES)
    got = dict(zip(GRID_QUERIES, out["queries"]["queries"][base:base + len(GRID_QUERIES)]))
    for (n, cap, cpw, crowded, slots), grid in got.items():
        if cpw > 0:
            assert grid == min(-(-n // cpw), cap)
        elif not crowded or n <= cap:
            assert grid == min(n, cap)
        else:
            assert grid % 32 == 0 or grid == cap
            assert min(32, cap) <= grid <= cap
            assert grid == min(cap, max(32, (n // slots + 16) // 32 * 32))
    assert out["whole_crowded_522"]["whole"]["grid"] == 128 and out["whole_crowded_522"]["whole"]["slots"] == 4      # 4 x 128
    assert out["whole_alone_522"]["whole"]["grid"] == 256 and out["whole_alone_522"]["whole"]["slots"] == 2          # 2 x 256
    assert out["whole_cpw"]["whole"]["grid"] == 174
    assert out["whole_alone_522"]["whole"]["order"] == list(range(522))


def test_whole_donate(out):
    base = len(LAT_QUERIES) + len(GRID_QUERIES)
    got = dict(zip(DONATE_QUERIES, out["queries"]["queries"][base:base + len(DONATE_QUERIES)]))
    for (d, b, ncl, grid), donate in got.items():
        assert donate == (int(b <= 1 and ncl > grid) if d < 0 else int(d != 0))
    assert out["whole_alone_522"]["whole"]["donate"] == 1
    assert out["whole_two_in_flight_522"]["whole"]["donate"] == 0
    assert out["whole_donate_never"]["whole"]["donate"] == 0
    assert out["whole_donate_always"]["whole"]["donate"] == 1
    assert out["auto_52"]["whole"]["donate"] == 0             # alone, but every cluster has a workgroup
    assert out["mode_cluster"]["whole"]["donate"] == 0        # k_icp_cluster hands nothing over


def test_pipe_slots(out):
    base = len(LAT_QUERIES) + len(GRID_QUERIES) + len(DONATE_QUERIES)
    got = dict(zip(SLOTS_QUERIES, out["queries"]["queries"][base:]))
    assert len(got) == len(SLOTS_QUERIES)
    for (s, b, grouped), slots in got.items():
        if s > 0:
            assert slots == min(s, CD_PIPE_SLOTS)
        else:
            assert slots == (CD_PIPE_SLOTS if b >= 4 and not grouped else 2)
    assert out["grouped_mixed5_crowded"]["grouped"]["slots"] == 2 and out["grouped_mixed5_slots3"]["grouped"]["slots"] == 3


def test_plane_grid_and_poll_groups(out):
    got = out["queries_unrecorded"]["queries"]
    for (no, cap), grid in zip(PLANE_GRID_QUERIES, got):
        assert grid == max(1, min(no, 2 * cap))       # two workgroups per CU at the most, one per cluster, at least one
    assert got[len(PLANE_GRID_QUERIES):] == [8, 16, 16, 16]


# ---- persist_launch ----------------------------------------------------------------------------------------------------------
def test_persist_launch(out):
    pe = {name: out[name]["persist"] for name in ALL_CASES if name.startswith("persist_")}
    assert pe["persist_8"] == {"launch": 1, "G": 14, "n_open": 7}          # eight clusters, one of them pre-marked: seven have tiles
    for name in ("persist_9", "persist_off", "persist_siblings", "persist_nwork_G_plus_1", "persist_no_work"):
        assert pe[name]["launch"] == 0, name
    assert plan(out, "persist_no_work")["nwork"] == 0
    assert pe["persist_siblings_forced"]["launch"] == 1
    assert plan(out, "persist_nwork_G")["nwork"] == 6 and pe["persist_nwork_G"] == {"launch": 1, "G": 6, "n_open": 3}
    assert plan(out, "persist_nwork_G_plus_1")["nwork"] == 6 and plan(out, "persist_nwork_G_plus_1")["wg_cap"] == 5


# ---- repack_active -----------------------------------------------------------------------------------------------------------
def test_repack_active(out):
    o = out["repack"]
    assert [w[0] for w in o["work"]] == [0, 0, 0, 0, 1, 3, 3, 3, 4, 4]
    assert o["repack"] == {"all_done": 0, "active": [[0, 0], [0, 1], [0, 2], [0, 3]]}      # done in either slot: the items go
    assert out["repack_all_done"]["repack"] == {"all_done": 1, "active": []}
    assert out["repack_one_slot_open"]["repack"] == {"all_done": 0, "active": []}          # all-done needs both slots
    assert out["work_tiny"]["repack"]["active"] == out["work_tiny"]["work"]
