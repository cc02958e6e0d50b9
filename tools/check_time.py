"""Time of the batched model check on the bench's own batch shape, in one process
on one device: configs[2] (262,144 x uniform 3-SAT, n = 100, m = 426) generated
in HBM, solved by satmi_dpll_batch_device (SOUND, one model per instance), then

  (a) satmi_check_models_device on the solver's output pointers as they are
      (cap = 1, stride = n), and
  (b) the torch expression bench.py checks its models with (models_ok_for,
      copied here, not imported: an int8 [B, n + 1] scatter target, a gather per
      literal), on the same tensors,

alternating, each bracketed by HIP events on one stream, after WARMUP calls of
each, REPS repetitions.  (a) and (b) must agree on every SAT instance.  One JSON
line per repetition and a summary line: median ms per call, and for (a) the
bytes the pass has to move (the CSR once, the rows, the output) over that time,
as GB/s and as a share of the 8 TB/s HBM peak.  [--instances B] [--reps R]."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sat-mpi-stana-andrei_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from satmi import _capi, cnf  # noqa: E402
from satmi.check import check_device  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP = 3
CHUNK = 32768   # instances generated at a time (the generator sorts an int32 [B, m, k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    _capi.require_gpu()
    L = _capi.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, n, m, k = args.instances, 100, 426, 3
    parts = [cnf.uniform_ksat_device(min(CHUNK, B - b0), n, m, k, 4242 + b0, dev)[2] for b0 in range(0, B, CHUNK)]
    lits = torch.cat(parts)
    del parts
    icb = (torch.arange(B + 1, device=dev, dtype=torch.int64) * m).to(torch.int32)
    clb = (torch.arange(B * m + 1, device=dev, dtype=torch.int64) * k).to(torch.int32)
    nv = torch.full((B,), n, device=dev, dtype=torch.int32)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    counters = torch.zeros((B, _capi.NCOUNTERS), dtype=torch.int64, device=dev)
    sol_len = torch.zeros(B, dtype=torch.int32, device=dev)
    sol_lits = torch.zeros((B, n), dtype=torch.int32, device=dev)
    out = torch.zeros((B, _capi.CHECK_NWORDS), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)

    def check():
        check_device(B, icb.data_ptr(), clb.data_ptr(), lits.data_ptr(), n, k, None, sol_len.data_ptr(),
                     sol_lits.data_ptr(), 1, n, out.data_ptr(), s.cuda_stream)

    def models_ok():   # bench.py's models_ok_for, on these tensors; returns the per-instance verdicts
        val = torch.zeros((B, n + 1), dtype=torch.int8, device=dev)
        live = torch.arange(n, device=dev)[None, :] < sol_len[:, None]
        idx = torch.where(live, sol_lits.abs(), 0).to(torch.int64)
        val.scatter_(1, idx, torch.where(sol_lits > 0, 1, -1).to(torch.int8))
        val[:, 0] = 0
        lv = lits.view(B, m, k).to(torch.int64)
        litval = torch.gather(val, 1, lv.abs().view(B, -1)).view(B, m, k) * torch.sign(lv).to(torch.int8)
        return (litval > 0).any(dim=2).all(dim=1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        r = fn()
        b.record(s)
        s.synchronize()
        return a.elapsed_time(b), r

    with torch.cuda.stream(s):
        rc = L.satmi_dpll_batch_device(B, icb.data_ptr(), clb.data_ptr(), lits.data_ptr(), nv.data_ptr(), n, m, m * k,
                                       k, None, None, _capi.MODE_SOUND, 1, 0, 0.0, 1, n, status.data_ptr(),
                                       counters.data_ptr(), sol_len.data_ptr(), sol_lits.data_ptr(), None, None,
                                       s.cuda_stream)
        _capi.check(rc, "satmi_dpll_batch_device")
        for _ in range(WARMUP):
            check()
            clause_ok = models_ok()
        s.synchronize()
        sat = counters[:, 5] > 0
        ours = (out[:, 0] == 0) & (out[:, 1] == 0) & (out[:, 3] == 0)
        agree = bool((ours[sat] == clause_ok[sat]).all().item()) and bool(ours[sat].all().item())
        nsat = int(sat.sum().item())
        row_bytes = 4 * int(sol_len.sum().item())
        t_check, t_torch = [], []
        for rep in range(args.reps):
            tc, _ = timed(check)
            tt, _ = timed(models_ok)
            t_check.append(tc)
            t_torch.append(tt)
            print(json.dumps({"rep": rep, "check_ms": round(tc, 4), "torch_ms": round(tt, 4)}), flush=True)
    if not agree:
        raise SystemExit("check_time: the check and the torch expression disagree on a SAT instance")
    csr_bytes = 4 * (B + 1) + 4 * (B * m + 1) + 4 * B * m * k
    moved = csr_bytes + 4 * B + row_bytes + 16 * B
    mc, mt = float(np.median(t_check)), float(np.median(t_torch))
    print(json.dumps({"instances": B, "n": n, "m": m, "k": k, "sat": nsat, "reps": args.reps, "agree": agree,
                      "check_ms_median": mc, "check_ms_min": min(t_check), "check_ms_max": max(t_check),
                      "torch_ms_median": mt, "torch_ms_min": min(t_torch), "torch_ms_max": max(t_torch),
                      "csr_gb": csr_bytes / 1e9, "moved_gb": moved / 1e9, "check_gb_per_s": moved / (mc * 1e-3) / 1e9,
                      "share_of_8tb_per_s": moved / (mc * 1e-3) / HBM_PEAK, "torch_over_check": mt / mc}), flush=True)


if __name__ == "__main__":
    main()
