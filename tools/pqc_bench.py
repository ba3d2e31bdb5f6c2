"""The split panel factorisation (CholeskyQR2 head pq_chol<true>, Householder reconstruction tail pq_tail) phase by
phase: one build of the library per phase of the head (tools/pqc_bench.sh build), each timed on a random m x 64 panel in
its own process; prints cumulative and per-phase times of the head, then one figure for the tail and one for the
one-kernel form (pq_chol<false>). Development tool. python tools/pqc_bench.py [m ...]"""
import sys, os, subprocess
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
child = r'''
import sys, os, ctypes as C
sys.path.insert(0, %r)
import bigkrls_amd._lib as L
L.LIB_PATH = sys.argv[1]
import bigkrls_amd as bk
ctx = bk.Context(0)
lib = L.load()
lib.bk_pqc_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]
lib.bk_pqc_bench.restype = C.c_int
out = []
for m in sys.argv[3:]:
    us = C.c_double()
    rc = lib.bk_pqc_bench(ctx.handle, int(m), 30, int(sys.argv[2]), C.byref(us), None)
    out.append("%%.1f" %% us.value)
print(" ".join(out))
''' % root
names = {1: "load", 2: "Gram 0", 3: "all-reduce 0", 4: "Cholesky 0", 5: "substitution 0", 6: "Gram 1", 7: "all-reduce 1",
         8: "Cholesky 1", 9: "substitution 1", 10: "stores of Q, R2 R1", 0: "LU of Q1 (whole head)"}
ms = sys.argv[1:] or ["512", "5120", "12000", "20000"]
print("m:".ljust(32) + "".join(f"{m:>16s}" for m in ms))


def run(ph, which):
    lib = os.path.join(root, "tools", "_ab", "pqc", f"libbigkrls_stop{ph}.so")
    r = subprocess.run([sys.executable, "-c", child, lib, str(which)] + ms, capture_output=True, text=True)
    try:
        return [float(x) for x in r.stdout.strip().split()[-len(ms):]]
    except Exception:
        print("failed:", r.stdout[-200:], r.stderr[-300:])
        return None


prev = [0.0] * len(ms)
for ph in list(range(1, 11)) + [0]:
    vals = run(ph, 0)
    if vals is None:
        continue
    print(f"head after {names[ph]:21s}" + "".join(f"{v:8.1f} (+{v - p:5.1f})" for v, p in zip(vals, prev)))
    prev = vals
for which, label in ((1, "tail (pq_tail) alone"), (2, "one-kernel form (whole)")):
    vals = run(0, which)
    if vals is not None:
        print(f"{label:32s}" + "".join(f"{v:8.1f}" + " " * 8 for v in vals))
