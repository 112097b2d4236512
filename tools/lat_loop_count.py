#!/usr/bin/env python3
"""Vector instructions per 64-query pass in the hot LAT_ITER loop of k_icp_lat - counted in the compiler's assembly, no GPU.

usage: python tools/lat_loop_count.py [--csrc DIR] [--keep FILE.s] [--json]

Compiles k_icp_lat.hip for the device with exactly the command perception_amd/csrc/Makefile uses for its object file (taken from
`make -n`, with -c replaced by -S --cuda-device-only) and, for k_icp_lat<4,2,false> and k_icp_lat<1,8,false>, walks the pass
loop of the LAT_ITER branch along the path a flagship batch takes:

  loop header -> [X <- T X and its store] -> nearest-neighbour block -> moment sums (the block with the 16 v_add_f64 of the
  fast fixed-point form) -> back edge.

 * Blocks are basic blocks: split at every label AND after every branch.  s_cbranch_execz is followed as not taken and
   s_cbranch_execnz as taken: the wave has lanes with a point, so the transform, its store and the sums are all on the path.
 * The nearest-neighbour block is the one with three v_cvt_rpi_i32_f32 (one per lat_axis call) that reaches a 16 x v_add_f64
   block inside the same loop; where a kernel holds several (one per face form: one-face-per-axis, three faces, six faces) the
   one with the FEWEST v_bfi_b32 is the taken one - the default template has three faces on three axes.
 * The loop is the one LLVM names in the block's "in Loop: Header=... Depth=..." comment; only blocks of that loop at that depth
   are walked, which leaves the tie walk (deeper loops) out.  Between the way points the path with the fewest vector
   instructions is taken (Dijkstra): that is the edge around the tie walk and its prologue.
 * The one s_cbranch_execz that IS followed is the one that jumps to the 16 x v_add_f64 block: it skips the other arm of that
   if / else, the out-of-range form of the moment sums, which no lane of a flagship batch takes.

A vector instruction is a line whose mnemonic starts with "v_" (VALU incl. compares, moves, lane reads); ds_ / global_ / s_ are
listed separately.  --csrc DIR counts another checkout's perception_amd/csrc (the parent commit's, for a before / after).

--solve reports the SOLVE instead (nothing else is compiled): a stand-alone probe with one kernel that calls the single-lane
icp_step and, where the checkout has icp_solve_row.hpp, one that calls icp_step_row on a row, compiled with the same command.
Per kernel, in layout order: the vector instructions before the sweep loop (the only loop that holds a v_sqrt_f32), inside it
and after it.  The sweep loop holds the three (p, q) pair bodies, so "rotation" = loop / 3: threshold test, rotation parameters,
the updates of W, U and V, a third of the loop control.  Every conditionally executed region is counted (both arms of t == 0 and
y == 0, the rank-2 branch after the loop) EXCEPT, in the row kernel, the plain form of row_rotation: the forward branch after the
validity test whose skipped region holds exactly the six IEEE divisions (v_div_fixup_f32) and three square roots of
jacobi_svd3's own statements - the largest such region of each pair.  Three are expected; anything else ends the tool with a
message.  The short form's own IEEE divisions (d / t and the one of tau) and square roots are listed, so that a build which lost
the short forms (-DCD_ROW_RCP_GE1=0, a compiler that expands them differently) shows as six divisions per rotation."""
import argparse
import heapq
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"<4,2,false>": "_ZN2cd9k_icp_latILi4ELi2ELb0EE", "<1,8,false>": "_ZN2cd9k_icp_latILi1ELi8ELb0EE"}
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)")


def compile_to_asm(csrc, out):
    """The Makefile's own compile line for k_icp_lat.o, turned into a device-only -S."""
    dry = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/k_icp_lat.o"], check=True, capture_output=True, text=True).stdout
    line = next(l for l in dry.splitlines() if "k_icp_lat.hip" in l and " -c " in l)
    argv = shlex.split(line)
    i = argv.index("-o")
    argv[i + 1] = out
    argv[argv.index("-c")] = "-S"
    argv.insert(1, "--cuda-device-only")
    subprocess.run(argv, check=True, cwd=csrc, stderr=subprocess.DEVNULL)


def parse_blocks(lines):
    """[(name, loop, insts, succs)]: loop = (header label, depth) from LLVM's comment or None; succs = names."""
    blocks, cur, anon = [], None, 0

    def start(name, loop):
        nonlocal cur
        cur = {"name": name, "loop": loop, "insts": [], "succ": [], "skip": [], "fall": True}
        blocks.append(cur)

    start("entry", None)
    last_loop = None
    for raw in lines:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", raw)
        if m:
            c = m.group(2)
            lm = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", c)
            if lm:
                last_loop = (".L" + lm.group(1), int(lm.group(2)))
            elif re.search(r"Loop Header|Parent Loop|=>This", c):
                last_loop = ("self:" + m.group(1), None)   # a header: resolved below
            else:
                last_loop = None
            start(m.group(1), last_loop)
            continue
        t = raw.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        cur["insts"].append(t)
        b = BRANCH.match(t)
        if b:
            # (on the taken path the wave has lanes: a branch on an EMPTY exec mask is never taken, one on a non-empty mask always)
            if b.group(1) != "s_cbranch_execz":
                cur["succ"].append(b.group(2))
            else:
                cur["skip"].append(b.group(2))
            if b.group(1) in ("s_branch", "s_cbranch_execnz"):
                cur["fall"] = False
            anon += 1
            start("%s+%d" % (cur["name"].split("+")[0], anon), cur["loop"])
        elif t.startswith("s_endpgm"):
            cur["fall"] = False
    for k, b in enumerate(blocks):
        if b["fall"] and k + 1 < len(blocks):
            b["succ"].append(blocks[k + 1]["name"])
    return blocks


def count(insts, prefix):
    return sum(1 for t in insts if t.startswith(prefix))


def dijkstra(blocks, allowed, src, dst, skip_to=None):
    """Cheapest path (vector instructions of the blocks entered) from src to dst inside `allowed`; returns the names after src."""
    by = {b["name"]: b for b in blocks}
    heap, best = [(0, src, ())], {}
    while heap:
        cost, name, path = heapq.heappop(heap)
        if name in best:
            continue
        best[name] = path
        if name == dst and path:
            return list(path)
        for s in by[name]["succ"] + [t for t in by[name]["skip"] if t == skip_to]:
            if s in by and (s in allowed) and (s not in best or s == dst):
                heapq.heappush(heap, (cost + count(by[s]["insts"], "v_"), s, path + (s,)))
    if dst in best and best[dst]:
        return list(best[dst])
    raise SystemExit("no path %s -> %s" % (src, dst))


def hot_path(asm_lines, mangled):
    i = next(k for k, l in enumerate(asm_lines) if l.startswith(mangled) and ":" in l)
    j = next(k for k in range(i, len(asm_lines)) if asm_lines[k].strip().startswith("s_endpgm"))
    blocks = parse_blocks(asm_lines[i + 1:j + 1])
    by = {b["name"]: b for b in blocks}

    def loop_of(b):   # (header, depth) for members; a header names itself, depth from its members
        return b["loop"]

    near = [b for b in blocks if count(b["insts"], "v_cvt_rpi_i32_f32") == 3 and loop_of(b) and loop_of(b)[1]]
    cands = []
    for h in near:
        hdr, depth = loop_of(h)
        allowed = {b["name"] for b in blocks if b["loop"] == (hdr, depth)} | {hdr} | {b["name"] for b in blocks if b["name"].startswith(hdr + "+")}
        moms = [b for b in blocks if b["name"] in allowed and count(b["insts"], "v_add_f64") >= 16]
        if moms:
            cands.append((count(h["insts"], "v_bfi_b32"), h, hdr, allowed, moms[0]))
    if not cands:
        raise SystemExit("no LAT_ITER pass loop found in " + mangled)
    cands.sort(key=lambda c: c[0])
    bfi, h, hdr, allowed, mom = cands[0]
    # a nearest-neighbour evaluation may be spread over several blocks (uniform branches inside it): walk from the header
    path = [hdr] + dijkstra(blocks, allowed, hdr, h["name"])
    path += dijkstra(blocks, allowed, h["name"], mom["name"], skip_to=mom["name"].split("+")[0])
    path += dijkstra(blocks, allowed, mom["name"], hdr)[:-1]
    insts = [t for n in path for t in by[n]["insts"]]
    # the path is the one meant: one fast moment form (16 conversions + 16 additions in double) and the face code of ONE form
    # (no mask selects, or the three-face loop's 15) - a merge or split of blocks by a later compiler would show here
    nf64, nbfi = sum(1 for t in insts if t.startswith("v_") and "f64" in t.split()[0]), count(insts, "v_bfi_b32")
    if nf64 != 32 or nbfi not in (0, 15) or count(insts, "v_cvt_rpi_i32_f32") != 3:
        raise SystemExit("%s: the walked path is not one LAT_ITER pass (%d f64, %d v_bfi_b32, %d v_cvt_rpi): look at the assembly" % (
            mangled, nf64, nbfi, count(insts, "v_cvt_rpi_i32_f32")))
    return {"blocks": path, "valu": count(insts, "v_"), "v_bfi_b32": count(insts, "v_bfi_b32"), "v_cndmask": count(insts, "v_cndmask"),
            "v_cmp": count(insts, "v_cmp"), "v_f64": sum(1 for t in insts if t.startswith("v_") and "f64" in t.split()[0]),
            "v_mov": count(insts, "v_mov"), "lds": count(insts, "ds_"), "global": count(insts, "global_"),
            "salu": count(insts, "s_") - count(insts, "s_waitcnt") - count(insts, "s_nop"), "exec_writes": sum(1 for t in insts if "saveexec" in t),
            "other_nearest_blocks_v_bfi": [c[0] for c in cands[1:]]}


SOLVE_PROBE = r"""
#include "icp_solve.hpp"
#if __has_include("icp_solve_row.hpp")
#include "icp_solve_row.hpp"
#define HAVE_ROW 1
#endif
using namespace cd;
extern "C" __global__ void __launch_bounds__(64) probe_lane(IcpState* st, const unsigned long long* A, const int* n, IcpParams prm, int* done) {
    __shared__ IcpState so;
    __shared__ unsigned long long a[16];
    if (threadIdx.x < 16) a[threadIdx.x] = A[blockIdx.x * 16 + threadIdx.x];
    if (threadIdx.x == 0) {
        so = st[blockIdx.x];
        done[blockIdx.x] = icp_step<false>(so, a, n[blockIdx.x], prm);
        st[blockIdx.x] = so;
    }
}
#ifdef HAVE_ROW
extern "C" __global__ void __launch_bounds__(64) probe_row(IcpState* st, const unsigned long long* A, const int* n, IcpParams prm, int* done) {
    __shared__ IcpState so;
    const int tid = (int)threadIdx.x;
    if (tid >= 16) return;
    if (tid == 0) so = st[blockIdx.x];
    RowLanes row(tid);
    RowLanes::V<unsigned long long> a;
    a.v = A[blockIdx.x * 16 + tid];
    const int d = icp_step_row<false>(row, so, a, n[blockIdx.x], prm);
    if (tid == 0) { done[blockIdx.x] = d; st[blockIdx.x] = so; }
}
#endif
"""


def compile_probe(csrc, src, out):
    """The Makefile's compile line for k_icp_lat.o with the probe as the source, device-only -S."""
    dry = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/k_icp_lat.o"], check=True, capture_output=True, text=True).stdout
    line = next(l for l in dry.splitlines() if "k_icp_lat.hip" in l and " -c " in l)
    argv = shlex.split(line)
    argv[argv.index("-o") + 1] = out
    argv[argv.index("-c")] = "-S"
    argv[argv.index("k_icp_lat.hip")] = src
    argv[1:1] = ["--cuda-device-only", "-I", csrc]
    subprocess.run(argv, check=True, cwd=csrc, stderr=subprocess.DEVNULL)


def solve_counts(asm_lines, kernel, skip_plain):
    i = next((k for k, l in enumerate(asm_lines) if l.startswith(kernel + ":")), None)
    if i is None:
        return None
    j = next(k for k in range(i, len(asm_lines)) if asm_lines[k].strip().startswith("s_endpgm"))
    blocks = parse_blocks(asm_lines[i + 1:j + 1])
    pos = {b["name"]: k for k, b in enumerate(blocks)}
    hdrs = {b["loop"][0] for b in blocks if b["loop"] and b["loop"][1] and count(b["insts"], "v_sqrt_f32")}
    if len(hdrs) != 1:
        raise SystemExit("%s: expected ONE loop with square roots (the sweeps), found %s: look at the assembly" % (kernel, sorted(hdrs)))
    hdr = hdrs.pop()
    inside = [k for k, b in enumerate(blocks) if (b["loop"] and b["loop"][0] == hdr) or b["name"].split("+")[0] == hdr]
    first, last = min(inside), max(inside)
    n = lambda ks, pre: sum(count(blocks[k]["insts"], pre) for k in ks)
    skipped = set()
    if skip_plain:
        regions = []
        for k in range(first, last + 1):
            for t in blocks[k]["insts"]:
                m = BRANCH.match(t)
                if m and m.group(1) != "s_branch" and pos.get(m.group(2), -1) > k + 1:
                    r = range(k + 1, pos[m.group(2)])
                    if n(r, "v_div_fixup_f32") == 6 and n(r, "v_sqrt_f32") == 3:
                        regions.append(r)
        regions = [r for r in regions if not any(o is not r and o.start <= r.start and r.stop <= o.stop for o in regions)]
        if len(regions) != 3:
            raise SystemExit("%s: expected the plain form of row_rotation three times, found %d regions: look at the assembly" % (kernel, len(regions)))
        for r in regions:
            skipped.update(r)
    loop = [k for k in range(first, last + 1) if k not in skipped]
    part = lambda ks: {"valu": n(ks, "v_"), "v_div_fixup_f32": n(ks, "v_div_fixup_f32"), "v_div_fixup_f64": n(ks, "v_div_fixup_f64"),
                       "v_sqrt_f32": n(ks, "v_sqrt_f32"), "v_rcp_f32": n(ks, "v_rcp_f32"), "ds_bpermute": n(ks, "ds_bpermute"),
                       "salu": n(ks, "s_") - n(ks, "s_waitcnt") - n(ks, "s_nop")}
    out = {"before": part(range(0, first)), "loop": part(loop), "after": part(range(last + 1, len(blocks))), "plain_form_skipped": part(sorted(skipped))}
    out["rotation"] = {k: v / 3.0 for k, v in out["loop"].items()}
    return out


def solve_report(csrc, keep):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "solve_probe.hip")
        open(src, "w").write(SOLVE_PROBE)
        out = os.path.abspath(keep) if keep else os.path.join(tmp, "solve_probe.s")
        compile_probe(csrc, src, out)
        lines = open(out).read().split("\n")
    res = {"lane": solve_counts(lines, "probe_lane", False)}
    row = solve_counts(lines, "probe_row", True)
    if row is not None:
        res["row"] = row
    return res


def resources(asm_lines):
    """vgprs / sgprs / spills / scratch / LDS of every k_icp_lat instantiation, from the .amdhsa metadata."""
    out, cur = {}, None
    for l in asm_lines:
        m = re.match(r"\s+\.name:\s+(_ZN2cd9k_icp_latILi(\d+)ELi(\d+)ELb([01])EE\S*)", l)
        if m:
            cur = "<%s,%s,%s>" % (m.group(2), m.group(3), "bounded" if m.group(4) == "1" else "unbounded")
            out[cur] = {}
            continue
        m = re.match(r"\s+\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", l)
        if m and cur is not None:
            out[cur].setdefault(m.group(1), int(m.group(2)))
        if l.strip().startswith(".name:") and "k_icp_lat" not in l:
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "perception_amd", "csrc"))
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--solve", action="store_true", help="report the solve (icp_step / icp_step_row) instead of the pass loop")
    a = ap.parse_args()
    if a.solve:
        res = {"solve": solve_report(os.path.abspath(a.csrc), a.keep)}
        if a.json:
            print(json.dumps(res))
            return 0
        for k, r in res["solve"].items():
            for part in ("before", "rotation", "after"):
                p = r[part]
                print("%-4s %-8s vector instructions %6.1f (IEEE f32 divisions %.1f, f64 %.1f, v_sqrt_f32 %.1f, v_rcp_f32 %.1f), ds_bpermute %.1f, scalar %.1f" % (
                    k, part, p["valu"], p["v_div_fixup_f32"], p["v_div_fixup_f64"], p["v_sqrt_f32"], p["v_rcp_f32"], p["ds_bpermute"], p["salu"]))
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.abspath(a.keep) if a.keep else os.path.join(tmp, "k_icp_lat.s")
        compile_to_asm(os.path.abspath(a.csrc), out)
        lines = open(out).read().split("\n")
    res = {"loop": {k: hot_path(lines, v) for k, v in KERNELS.items()}, "resources": resources(lines)}
    if a.json:
        print(json.dumps(res))
        return 0
    for k, r in res["loop"].items():
        print("k_icp_lat%s LAT_ITER pass, taken path: %d vector instructions (v_cndmask %d, v_cmp %d, v_bfi_b32 %d, f64 %d, v_mov %d), "
              "%d LDS, %d global, %d scalar, %d exec-mask saves; %d blocks" % (k, r["valu"], r["v_cndmask"], r["v_cmp"], r["v_bfi_b32"], r["v_f64"],
                                                                              r["v_mov"], r["lds"], r["global"], r["salu"], r["exec_writes"], len(r["blocks"])))
    for k in sorted(res["resources"]):
        r = res["resources"][k]
        print("k_icp_lat%-16s vgpr %3d sgpr %3d vgpr spills %d sgpr spills %2d scratch %d B LDS %5d B" % (
            k, r.get("vgpr_count", -1), r.get("sgpr_count", -1), r.get("vgpr_spill_count", -1), r.get("sgpr_spill_count", -1),
            r.get("private_segment_fixed_size", -1), r.get("group_segment_fixed_size", -1)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
