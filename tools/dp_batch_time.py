"""Batched against single-call Davis-Putnam elimination on small random 3-SAT
sets, in one process on one device: for the bench's own rand-dp set (16
formulas, n = 16, m = 96, seed 7002) and for 4,096 formulas of the same
distribution,
  (a) one eliminate_batch call (an UNFIT formula counts, with its rerun),
  (b) a loop of eliminate calls,
  (c) that loop from 8 threads (the workspace pool overlaps the calls),
each after a warm-up call of its form, 5 repetitions, the median and the
spread (min .. max) reported; all three must give equal `result`, `vars` and
`steps` for every formula.  Beside them the C call of (a) alone.  One JSON
line per set; [tag] in argv.

--sweep: the C call alone on both sets at workgroup widths 64 .. 1024 (the
SATMI_DP_BATCH_WIDTH knob of csrc/dp_batch.hip) and, for the large set, at the
1,024-clause capacity beside the tier's 1,920 (satmi_dp_debug_batch)."""
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sat-mpi-stana-andrei_amd'))
import numpy as np  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.dp import debug_batch, eliminate, eliminate_batch  # noqa: E402
from satmi.resolution import _p  # noqa: E402

REPS = 5


def timed(fn):
    fn()   # warm-up
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), (min(ts), max(ts)), out


def c_call(L, cb, scap=64):
    B = cb.num_instances
    res, steps = np.zeros(B, np.int32), np.zeros(B, np.int32)
    tr, sc = np.zeros((B, scap), np.int32), np.zeros((B, scap), np.int64)
    rc = L.satmi_dp_batch_host(B, _p(cb.inst_clause_begin), _p(cb.clause_lit_begin), _p(cb.lits), 0, 0,
                               _p(res), _p(steps), _p(tr), _p(sc, ctypes.c_int64), scap, None, 0, None, 0, None)
    _capi.check(rc, "satmi_dp_batch_host")
    return res, sc


def sweep(L, tag):
    for B in (16, 4096):
        cb = cnf.uniform_ksat(B, 16, 96, 3, seed=7002)
        for cap in ((0,) if B == 16 else (0, 1024)):
            debug_batch(0, cap)
            for w in (0, 64, 128, 256, 512, 1024):
                if w:
                    os.environ["SATMI_DP_BATCH_WIDTH"] = str(w)
                else:
                    os.environ.pop("SATMI_DP_BATCH_WIDTH", None)
                t, (lo, hi), (res, sc) = timed(lambda: c_call(L, cb))
                print(json.dumps({"tag": tag, "formulas": B, "clause_cap": cap or "tier", "width": w or "tier",
                                  "batch_c_call_ms": t * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3,
                                  "formulas_per_s": B / t, "unfit": int((res == _capi.DP_BATCH_UNFIT).sum()),
                                  "max_list": int(sc.max())}), flush=True)
    os.environ.pop("SATMI_DP_BATCH_WIDTH", None)
    debug_batch(0, 0)


def main():
    L = _capi.load()
    tag = " ".join(a for a in sys.argv[1:] if not a.startswith("--"))
    if "--sweep" in sys.argv:
        return sweep(L, tag)
    pool = ThreadPoolExecutor(8)
    for B in (16, 4096):
        cb = cnf.uniform_ksat(B, 16, 96, 3, seed=7002)
        fs = [cb.instance(b) for b in range(B)]
        ta, sa, ra = timed(lambda: eliminate_batch(cb))
        tb, sb, rb = timed(lambda: [eliminate(f) for f in fs])
        tc, sc_, rc = timed(lambda: list(pool.map(eliminate, fs)))
        tcc, scc, (res, _) = timed(lambda: c_call(L, cb))
        for x, y, z in zip(ra, rb, rc):
            assert (x["result"], x["vars"], x["steps"]) == (y["result"], y["vars"], y["steps"]) \
                == (z["result"], z["vars"], z["steps"])
        ms = lambda s: [s[0] * 1e3, s[1] * 1e3]   # noqa: E731
        print(json.dumps({
            "tag": tag, "formulas": B, "unfit": sum(r["path"] != "batch" for r in ra),
            "batch_ms": ta * 1e3, "batch_min_max_ms": ms(sa), "loop_ms": tb * 1e3, "loop_min_max_ms": ms(sb),
            "loop_8_threads_ms": tc * 1e3, "loop_8_threads_min_max_ms": ms(sc_),
            "batch_c_call_ms": tcc * 1e3, "batch_c_call_min_max_ms": ms(scc),
            "batch_formulas_per_s": B / ta, "loop_formulas_per_s": B / tb, "loop_8_threads_formulas_per_s": B / tc,
            "batch_over_loop": tb / ta, "batch_over_8_threads": tc / ta,
            "batch_over_8_threads_worst_case": sc_[0] / sa[1],
            "max_list": max(max(r["step_clauses"], default=0) for r in ra if r["path"] == "batch"),
            "sat": sum(r["result"] == 1 for r in ra)}), flush=True)
    pool.shutdown()


if __name__ == "__main__":
    main()
