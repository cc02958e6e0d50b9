"""Time of the batched refutation check on the bench's rand-res shape, in one
process on one device: configs[3]'s 16 random 3-SAT formulas (n = 7, m = 49,
seed 7001, drawn as bench.py draws them) saturated by resolve_batch(record=True),
their records turned into proofs (proof_of_resolution), then

  (a) satmi_check_refutations_device on the two CSR triples in device memory,
      bracketed by HIP events on one stream: WARMUP calls, then REPS repetitions,
  (b) the resolve_batch(record=True) call that produced the proofs (host clock
      around the call, which ends in a device synchronise), same repetitions,
  (c) the plain Python evaluator of tests/refute_rows.py on the same proofs, once
      (host clock).

The check's words must equal the evaluator's.  One JSON line per repetition and
a summary line: median / min / max ms of (a) and (b), the seconds of (c), the
clause form (a) ran in, the lemmas and literals checked.  [--reps R]
[--max-clause-len L]  (L = 0 runs the wave-per-clause form)."""
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
import refute_rows as rr  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.refute import check_refutations_device, proof_of_resolution  # noqa: E402
from satmi.resolution import resolve_batch  # noqa: E402

WARMUP = 3
COUNT, N, M, SEED = 16, 7, 49, 7001   # bench.py's RANDSETS["rand-res"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-clause-len", type=int, default=-1, help="-1 = the true one")
    args = ap.parse_args()
    _capi.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    batch = cnf.uniform_ksat(COUNT, N, M, 3, seed=SEED)
    fs = [batch.instance(b) for b in range(COUNT)]

    t_solve = []
    for rep in range(WARMUP + args.reps):
        t0 = time.perf_counter()
        rs = resolve_batch(batch, record=True)
        if rep >= WARMUP:
            t_solve.append((time.perf_counter() - t0) * 1e3)
    proofs = [proof_of_resolution(r) for r in rs]
    pb = cnf.pack(proofs)
    lemmas, lits = int(pb.inst_clause_begin[-1]), int(pb.clause_lit_begin[pb.inst_clause_begin[-1]])
    true_len = max(len(c) for f in fs + proofs for c in f)
    mcl = true_len if args.max_clause_len < 0 else args.max_clause_len
    form = "lane-per-clause" if 1 <= mcl <= rr.SHORT_MAX else "wave-per-clause"

    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in
         (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits,
          pb.inst_clause_begin, pb.clause_lit_begin, pb.lits)]
    out = torch.zeros((COUNT, _capi.REFUTE_NWORDS), dtype=torch.int32, device=dev)
    ok = torch.zeros(max(lemmas, 1), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)

    def check():
        check_refutations_device(COUNT, *(x.data_ptr() for x in t), N, mcl, out.data_ptr(), ok.data_ptr(),
                                 s.cuda_stream)

    t_check = []
    with torch.cuda.stream(s):
        for rep in range(WARMUP + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            check()
            b.record(s)
            s.synchronize()
            if rep >= WARMUP:
                t_check.append(a.elapsed_time(b))
                print(json.dumps({"rep": rep - WARMUP, "check_ms": round(t_check[-1], 4),
                                  "resolve_batch_ms": round(t_solve[rep - WARMUP], 4)}), flush=True)
    t0 = time.perf_counter()
    want_words, want_ok = rr.expected(fs, proofs, N)
    t_eval = time.perf_counter() - t0
    agree = out.cpu().numpy().tolist() == want_words and ok.cpu().numpy()[:lemmas].tolist() == want_ok
    if not agree:
        raise SystemExit("refute_time: the check and the Python evaluator disagree")
    verdicts = [r["result"] for r in rs]
    print(json.dumps({"formulas": COUNT, "n": N, "m": M, "seed": SEED, "unsat": verdicts.count(0),
                      "sat": verdicts.count(1), "proven": int((out[:, 0] == _capi.REFUTE_PROVEN).sum().item()),
                      "lemmas": lemmas, "lemma_literals": lits, "max_clause_len": mcl, "form": form,
                      "reps": args.reps, "agree": agree,
                      "check_ms_median": float(np.median(t_check)), "check_ms_min": min(t_check),
                      "check_ms_max": max(t_check),
                      "resolve_batch_ms_median": float(np.median(t_solve)), "resolve_batch_ms_min": min(t_solve),
                      "resolve_batch_ms_max": max(t_solve),
                      "python_evaluator_s": t_eval}), flush=True)


if __name__ == "__main__":
    main()
