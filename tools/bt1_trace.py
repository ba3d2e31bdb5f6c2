"""Reads a kernel trace of a fit (rocprofv3 --kernel-trace, csv) and reports the stage-1 back-transform of the dense
eigensolver: the launches between the last bt2_* kernel of a decomposition and the first kernel after them that is
neither gemm_kernel nor splitk_reduce_kernel. Per fit: the span, the time inside kernels, and per product of a step
(p1 = gemm_kernel<true, false, *>, its splitk_reduce_kernel, p2 and p3 = the two gemm_kernel<false, false, *> behind
it) the instantiation, the number of launches, and the mean, minimum and sum of their durations. Development tool.

    python tools/bt1_trace.py TRACE_kernel_trace.csv
"""
import collections
import csv
import re
import sys


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    names = [r[2] for r in rows]
    is_bt2 = [re.search(r"\bbt2_\w+", n) is not None for n in names]
    is_thin = [("gemm_kernel<" in n) or ("splitk_reduce_kernel" in n) for n in names]
    fits = []
    i = 0
    while i < len(rows):
        if is_bt2[i] and (i + 1 == len(rows) or not is_bt2[i + 1]):
            j = i + 1
            while j < len(rows) and is_thin[j]:
                j += 1
            if j - i - 1 >= 3:
                fits.append((i + 1, j))
            i = j
        else:
            i += 1
    print(f"{path}: {len(rows)} launches, {len(fits)} stage-1 back-transforms")
    for k, (a, b) in enumerate(fits):
        seg = rows[a:b]
        span = (seg[-1][1] - rows[a - 1][1]) / 1e3
        busy = sum(e - s for s, e, _ in seg) / 1e3
        stat = collections.OrderedDict()
        role, nn = None, 0
        for s, e, n in seg:
            m = re.search(r"gemm_kernel<(\w+), (\w+), (\d+)", n)
            if m and m.group(1) == "true":
                role, nn = "p1 Vb'Zs  ", 0
            elif m:
                nn += 1
                role = "p2 Tb W1  " if nn == 1 else "p3 Zs-=VbW"
            else:
                role = "p1 reduce "
            key = (role, f"gemm_kernel<{m.group(1)}, {m.group(2)}, {m.group(3)}>" if m else "splitk_reduce_kernel")
            stat.setdefault(key, []).append((e - s) / 1e3)
        print(f"fit {k}: {b - a} launches, span {span:.1f} us after the last bt2 kernel, {busy:.1f} us inside kernels, "
              f"{span - busy:.1f} us between them")
        for (role, kern), d in stat.items():
            print(f"    {role} {kern:36s} n={len(d):3d}  mean {sum(d) / len(d):7.1f}  min {min(d):7.1f}  sum {sum(d):8.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
