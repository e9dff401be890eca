"""Per-launch averages of the tap-GEMM kernels in a rocprofv3 --kernel-trace run (rocpd sqlite), one row per (kernel, grid, workgroup):
the same template runs at 64 and at 128 channels, and only the grid tells the two apart.

    python profiles/summarize_per_launch.py <results.db> [name-regex]
"""
import re
import sqlite3
import sys


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"^void ", "", re.sub(r"\(.*$", "", name))[:70]


def main(path, pat=r"^tap(gemm|stream)_kernel"):
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    dims = [c for c in cols if re.search(r"^(grid|workgroup)(_size)?_?[xy]$", c, re.I)]
    if not dims:
        print("# no grid columns among %s" % cols)
    agg = {}
    for row in cur.execute("select %s, start, end%s from kernels" % (name_col, "".join(", " + c for c in dims))):
        k = short(row[0])
        if not re.search(pat, k):
            continue
        a = agg.setdefault((k,) + tuple(row[3:]), [])
        a.append(row[2] - row[1])
    print("# %s" % path)
    print("%-72s %-22s %6s %9s %9s %9s %9s" % ("kernel", "/".join(dims), "calls", "avg_us", "median_us", "min_us", "max_us"))
    for key, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        v.sort()
        print("%-72s %-22s %6d %9.2f %9.2f %9.2f %9.2f" % (key[0], "/".join(str(d) for d in key[1:]), len(v), sum(v) / len(v) / 1e3,
                                                         v[len(v) // 2] / 1e3, v[0] / 1e3, v[-1] / 1e3))


if __name__ == "__main__":
    main(*sys.argv[1:3])
