"""Time of the batched witness reconstruction, in one process on one device, on the
records of two of configs[3]'s random 3-SAT sets, drawn as bench.py draws them:
rand-dp (16 formulas, n = 16, m = 96, seed 7002) through eliminate_batch and
rand-res (16 formulas, n = 7, m = 49, seed 7001) through resolve_batch, both with
record=True.  Only a True answer has a witness, and at these ratios nearly every
formula is unsatisfiable: a set with fewer than MIN_TRUE True answers is replaced by
its variant at the same count, n and seed with m = 3 n clauses, and the line says so.

Per set: the solve call that made the records (host clock around the call, which
ends in a synchronise), the plain Python rule of tests/witness_rows.py on the same
instances (host clock), and satmi_witness_models_device on the arrays in device
memory, bracketed by HIP events on one stream, WARMUP calls then REPS repetitions,
forced through each clause form (max_clause_len 8 = lane-per-clause, 0 = wave-per-clause).
Every word and row must equal the rule's, and every instance must be a MODEL.
One JSON line per set and form.  [--reps R]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-mpi-stana-andrei_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import witness_rows as wr  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.dp import eliminate_batch  # noqa: E402
from satmi.resolution import resolve_batch  # noqa: E402
from satmi.witness import (record_of, stages_of_elimination, stages_of_resolution,  # noqa: E402
                           witness_models_device)

WARMUP = 3
MIN_TRUE = 4
SETS = (("rand-dp", 16, 16, 96, 7002, eliminate_batch, stages_of_elimination, False),
        ("rand-res", 16, 7, 49, 7001, resolve_batch, stages_of_resolution, True))   # bench.py's RANDSETS


def solved(count, n, m, seed, solve):
    batch = cnf.uniform_ksat(count, n, m, 3, seed=seed)
    solve(batch, record=True)   # (the first call loads the code object)
    t0 = time.perf_counter()
    rs = solve(batch, record=True)
    return batch, rs, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    _capi.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = torch.cuda.Stream(dev)
    for name, count, n, m, seed, solve, build, ho in SETS:
        batch, rs, solve_ms = solved(count, n, m, seed, solve)
        variant = sum(r["result"] == 1 for r in rs) < MIN_TRUE
        if variant:
            m = 3 * n
            batch, rs, solve_ms = solved(count, n, m, seed, solve)
        true = [b for b, r in enumerate(rs) if r["result"] == 1]
        fs = [batch.instance(b) for b in true]
        recs = [record_of(rs[b]) for b in true]
        sts = [build(f, rs[b]) for f, b in zip(fs, true)]
        B = len(fs)
        t0 = time.perf_counter()
        want = wr.expected(fs, recs, sts, ho, n, n)
        python_ms = (time.perf_counter() - t0) * 1e3
        fb, rb = cnf.pack(fs), cnf.pack(recs)
        isb = np.cumsum([0] + [len(x) for x in sts])
        flat = np.array([t for x in sts for t in x], dtype=np.int64).reshape(-1, 3)
        host = [fb.inst_clause_begin, fb.clause_lit_begin, fb.lits, rb.inst_clause_begin, rb.clause_lit_begin, rb.lits,
                isb, flat[:, 0], flat[:, 1], flat[:, 2]]
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in host]
        out = torch.zeros((B, _capi.WITNESS_NWORDS), dtype=torch.int32, device=dev)
        lens = torch.zeros(B, dtype=torch.int32, device=dev)
        rows = torch.zeros((B, n), dtype=torch.int32, device=dev)
        true_len = max(len(c) for f in fs + recs for c in f)
        clauses, rec_clauses = int(fb.inst_clause_begin[-1]), int(rb.inst_clause_begin[-1])
        # clause reads of the stages: what a highest_only stage costs is the whole set, once per variable
        reads = sum(hi - lo for x in sts for _, lo, hi in x)
        # (the lane-per-clause form is right at any length, a lane walks its clause alone: 8 forces it)
        for mcl in (wr.SHORT_MAX, 0):
            ms = []
            with torch.cuda.stream(s):
                for rep in range(WARMUP + args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    witness_models_device(B, *(x.data_ptr() for x in t), ho, n, mcl, out.data_ptr(), lens.data_ptr(),
                                          rows.data_ptr(), n, s.cuda_stream)
                    b.record(s)
                    s.synchronize()
                    if rep >= WARMUP:
                        ms.append(a.elapsed_time(b))
            hl, hr = lens.cpu().numpy().tolist(), rows.cpu().numpy()
            got = (out.cpu().numpy().tolist(), hl, [hr[b, :hl[b]].tolist() for b in range(B)])
            assert got == want, (name, mcl)
            assert all(w == [wr.MODEL, 0, -1, 0, 0, -1] for w in got[0]), (name, mcl)
            print(json.dumps({"set": name, "formulas": count, "n": n, "m": m, "seed": seed, "variant": variant,
                              "true": B, "highest_only": ho, "clauses": clauses, "record_clauses": rec_clauses,
                              "stages": int(isb[-1]), "stage_clause_reads": reads, "longest_clause": true_len, "max_clause_len": mcl,
                              "form": "lane-per-clause" if 1 <= mcl <= wr.SHORT_MAX else "wave-per-clause",
                              "reps": args.reps, "equals_rule": True, "all_models": True,
                              "witness_ms_median": float(np.median(ms)), "witness_ms_min": min(ms),
                              "witness_ms_max": max(ms), "solve_ms": round(solve_ms, 3),
                              "python_rule_ms": round(python_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
