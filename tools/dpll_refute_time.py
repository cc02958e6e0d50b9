"""Time of DPLL's refutation logging and of the check of what it logs, in one process
on one device, on one seeded set: COUNT uniform random 3-SAT formulas, n = 50,
alpha = 4.26 (m = 213), all in device memory.  Bracketed by HIP events on one stream,
WARMUP calls and then REPS repetitions each:

  (a) satmi_dpll_batch_device under SATMI_KERNEL_GENERAL: the unlogged general kernel,
  (b) satmi_dpll_refutations_device on the same inputs: the logging kernel and the pack,
  (c) satmi_check_refutations_device on the proof triple (b) wrote,
  (d) for scale, satmi_dpll_batch_device under the default policy (the bench kernel).

(a), (b) and (d) must agree on every status and counter (ticks excepted), and (c) must
prove exactly the instances that ended exhausted with no model.  One JSON line per
repetition and a summary line: median / min / max ms of each.  [--reps R] [--count B]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-mpi-stana-andrei_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.refute import check_refutations_device, dpll_refutations_device  # noqa: E402

WARMUP = 3
N, M, SEED = 50, 213, 4260


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count", type=int, default=4096)
    args = ap.parse_args()
    _capi.require_gpu()
    L = _capi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.count
    batch = cnf.uniform_ksat(B, N, M, 3, seed=SEED)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in
         (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits, batch.inst_nvars)]

    def outputs():
        z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)   # noqa: E731
        return dict(status=z(B), counters=z(B * 8, torch.int64), sol_len=z(B), sol_lits=z(B * N), root_len=z(B),
                    root_lits=z(B * N))
    plain, logd, auto = outputs(), outputs(), outputs()
    room = 1 << 14                                   # log words per instance; checked below against the counts
    ccap, lcap = 256 * B, 2048 * B
    log = torch.zeros(B * room, dtype=torch.int32, device=dev)
    lb = torch.arange(B + 1, dtype=torch.int64, device=dev) * room
    pib, pcb, plits = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (B + 1, ccap + 1, lcap))
    info, totals = torch.zeros(B * 4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    out = torch.zeros((B, _capi.REFUTE_NWORDS), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)

    def solve(o):
        rc = L.satmi_dpll_batch_device(B, *(x.data_ptr() for x in t), N, M, 3 * M, 3, None, None, _capi.MODE_SOUND,
                                       1, 0, 0.0, 1, N, *(o[k].data_ptr() for k in o), s.cuda_stream)
        _capi.check(rc, "satmi_dpll_batch_device")

    def solve_logged():
        dpll_refutations_device(B, *(x.data_ptr() for x in t), N, M, 3 * M, 3, *(logd[k].data_ptr() for k in logd),
                                1, N, log.data_ptr(), lb.data_ptr(), pib.data_ptr(), pcb.data_ptr(), ccap,
                                plits.data_ptr(), lcap, info.data_ptr(), totals.data_ptr(), stream=s.cuda_stream)

    def check():
        check_refutations_device(B, *(x.data_ptr() for x in t[:3]), pib.data_ptr(), pcb.data_ptr(), plits.data_ptr(),
                                 N, 0, out.data_ptr(), None, s.cuda_stream)

    def general():
        _capi.set_kernel(_capi.KERNEL_GENERAL)
        try:
            solve(plain)
        finally:
            _capi.set_kernel(_capi.KERNEL_AUTO)
    legs = (("general_ms", general), ("logged_ms", solve_logged), ("check_ms", check),
            ("default_policy_ms", lambda: solve(auto)))
    times = {k: [] for k, _ in legs}
    with torch.cuda.stream(s):
        for rep in range(WARMUP + args.reps):
            row = {}
            for name, leg in legs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                leg()
                b.record(s)
                s.synchronize()
                row[name] = round(a.elapsed_time(b), 4)
            if rep >= WARMUP:
                for k, v in row.items():
                    times[k].append(v)
                print(json.dumps(dict(rep=rep - WARMUP, **row)), flush=True)
    h = {k: (plain[k].cpu().numpy(), logd[k].cpu().numpy(), auto[k].cpu().numpy()) for k in ("status", "counters")}
    ctr = [c.reshape(B, 8)[:, :7] for c in h["counters"]]
    if not ((h["status"][0] == h["status"][1]).all() and (h["status"][0] == h["status"][2]).all()
            and (ctr[0] == ctr[1]).all() and (ctr[0] == ctr[2]).all()):
        raise SystemExit("dpll_refute_time: the logged, the general and the default-policy searches disagree")
    hi = info.cpu().numpy().reshape(B, 4)
    if hi[:, 2].any() or int(totals[0]) > ccap or int(totals[1]) > lcap:
        raise SystemExit("dpll_refute_time: a log or the proof arrays were too small")
    unsat = (h["status"][1] == _capi.DPLL_EXHAUSTED) & (ctr[1][:, 5] == 0)
    ho = out.cpu().numpy()
    if not ((ho[unsat, 0] == _capi.REFUTE_PROVEN).all() and (ho[~unsat, 0] == _capi.REFUTE_OPEN).all()
            and not ho[:, 1].any() and (hi[unsat, 0] == ctr[1][unsat, 1] + 1).all()):
        raise SystemExit("dpll_refute_time: the check does not prove exactly the UNSAT answers")
    summary = {"formulas": B, "n": N, "m": M, "seed": SEED, "unsat": int(unsat.sum()), "sat": int((~unsat).sum()),
               "proven": int((ho[:, 0] == _capi.REFUTE_PROVEN).sum()), "lemmas": int(totals[0]),
               "lemma_literals": int(totals[1]), "log_words_max": int(hi[:, 1].max()), "reps": args.reps}
    for k, v in times.items():
        summary.update({k + "_median": float(np.median(v)), k + "_min": min(v), k + "_max": max(v)})
    summary["logged_over_general"] = summary["logged_ms_median"] / summary["general_ms_median"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
