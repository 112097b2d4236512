#!/usr/bin/env python3
"""trace_ops.py DIR [--stream ID]: the ordered list of stream operations in a rocprofv3 run (--kernel-trace --memory-copy-trace
--output-format csv -d DIR), one line each: `K <kernel> grid X,Y,Z block X,Y,Z` or `C <direction> <bytes>` (`?` where the trace has no byte column), in the order the
host issued them (correlation id; start time where a trace has none).  Two builds that issue the same operations give the same
text, so `diff` of two outputs is the op-for-op check of a refactor of the host code.  Times are left out on purpose."""
import csv
import glob
import sys


def rows(d, suffix):
    out = []
    for f in sorted(glob.glob(d + "/**/*" + suffix, recursive=True)):
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    return out


def first(r, *names):
    for n in names:
        if r.get(n) not in (None, ""):
            return r[n]
    return "?"


def main():
    d = sys.argv[1]
    stream = sys.argv[sys.argv.index("--stream") + 1] if "--stream" in sys.argv else None
    ops = []
    for r in rows(d, "kernel_trace.csv"):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("cd::", "").split("<")[0]
        text = "K %s grid %s,%s,%s block %s,%s,%s" % (name, first(r, "Grid_Size_X", "Grid_Size"), first(r, "Grid_Size_Y"), first(r, "Grid_Size_Z"),
                                                     first(r, "Workgroup_Size_X", "Workgroup_Size"), first(r, "Workgroup_Size_Y"), first(r, "Workgroup_Size_Z"))
        ops.append((r, text))
    for r in rows(d, "memory_copy_trace.csv"):
        ops.append((r, "C %s %s" % (first(r, "Direction", "Name", "Kind").replace("MEMORY_COPY_", ""), first(r, "Bytes", "Size", "Copy_Bytes"))))
    if stream is not None:
        ops = [o for o in ops if o[0].get("Stream_Id") == stream]
    by_corr = all(o[0].get("Correlation_Id", "").isdigit() and int(o[0]["Correlation_Id"]) > 0 for o in ops)
    ops.sort(key=lambda o: (int(o[0]["Correlation_Id"]) if by_corr else 0, int(o[0]["Start_Timestamp"])))
    for _, text in ops:
        print(text)


if __name__ == "__main__":
    main()
