"""Batched against single-call resolution on small random UNSAT sets, in one
process on one device: for the bench's own rand-res set (16 formulas, n = 7,
m = 49, seed 7001) and for 4,096 formulas of the same distribution,
  (a) one resolve_batch call,
  (b) a loop of resolve calls,
  (c) that loop from 8 threads (the workspace pool overlaps the calls),
each after a warm-up call of its form, 5 repetitions, the median reported;
(a) and (b) must give equal `result` and `pass_new` for every formula.
Beside them the C call of (a) alone (the Python wrapper's share is the
difference).  One JSON line per set; [lib tag] in argv (SATMI_LIB_VARIANT
picks the library)."""
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sat-mpi-stana-andrei_amd'))
import numpy as np  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.resolution import _p, resolve, resolve_batch  # noqa: E402

REPS = 5


def median_s(fn):
    fn()   # warm-up
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def c_call(L, cb, pcap=32):
    B = cb.num_instances
    res, passes = np.zeros(B, np.int32), np.zeros(B, np.int32)
    pn = np.zeros((B, pcap), np.int64)
    rc = L.satmi_resolution_batch_host(B, _p(cb.inst_clause_begin), _p(cb.clause_lit_begin), _p(cb.lits), 0, 0,
                                       _p(res), _p(passes), _p(pn, ctypes.c_int64), pcap, None, 0, None, 0, None)
    _capi.check(rc, "satmi_resolution_batch_host")
    return res


def widths(L, tag):
    """--widths: the batched call alone on one set per capacity tier (the sets the
    workgroup widths were chosen on: build variants with -DSATMI_RB_WIDTH_*)."""
    for n, m, tier in ((4, 10, 256), (6, 26, 1024), (7, 49, 2560), (8, 20, 4096)):
        cb = cnf.uniform_ksat(4096, n, m, 3, seed=7001)
        t, res = median_s(lambda: c_call(L, cb))
        print(json.dumps({"lib": tag, "tier_keys": tier, "n": n, "m": m, "formulas": 4096, "batch_c_call_ms": t * 1e3,
                          "formulas_per_s": 4096 / t, "unfit": int((res == _capi.RES_BATCH_UNFIT).sum())}),
              flush=True)
    cb = cnf.uniform_ksat(16, 7, 49, 3, seed=7001)
    t, _ = median_s(lambda: c_call(L, cb))
    print(json.dumps({"lib": tag, "tier_keys": 2560, "n": 7, "m": 49, "formulas": 16, "batch_c_call_ms": t * 1e3,
                      "formulas_per_s": 16 / t}), flush=True)


def main():
    L = _capi.load()
    if "--widths" in sys.argv:
        return widths(L, " ".join(a for a in sys.argv[1:] if a != "--widths"))
    pool = ThreadPoolExecutor(8)
    for B in (16, 4096):
        cb = cnf.uniform_ksat(B, 7, 49, 3, seed=7001)
        fs = [cb.instance(b) for b in range(B)]
        ta, ra = median_s(lambda: resolve_batch(cb))
        tb, rb = median_s(lambda: [resolve(f) for f in fs])
        tc, rc = median_s(lambda: list(pool.map(resolve, fs)))
        tcc, res = median_s(lambda: c_call(L, cb))
        for x, y, z in zip(ra, rb, rc):
            assert (x["result"], x["pass_new"]) == (y["result"], y["pass_new"]) == (z["result"], z["pass_new"])
        assert res.tolist() == [x["result"] for x in ra]
        print(json.dumps({
            "lib": " ".join(sys.argv[1:]), "formulas": B, "unfit": sum(r["path"] != "batch" for r in ra),
            "batch_ms": ta * 1e3, "loop_ms": tb * 1e3, "loop_8_threads_ms": tc * 1e3, "batch_c_call_ms": tcc * 1e3,
            "batch_formulas_per_s": B / ta, "loop_formulas_per_s": B / tb, "loop_8_threads_formulas_per_s": B / tc,
            "batch_over_loop": tb / ta, "batch_over_8_threads": tc / ta,
            "clauses_derived": int(sum(sum(r["pass_new"]) for r in ra))}), flush=True)
    pool.shutdown()


if __name__ == "__main__":
    main()
