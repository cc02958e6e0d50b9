"""Time of the sound CDCL with carried lemmas (csrc/cdcl_sound.hip) in the manner of
tools/cdcl_assume_time.py: one process on one device, bracketed by HIP events on one stream,
WARMUP calls and then REPS repetitions each, on the 4,096 uniform random 3-SAT formulas at
n = 50, m = 213 of that tool (seed 4260):

  (a) overhead without a carry: satmi_cdcl_assume_batch_device with no assumptions against
      satmi_cdcl_carry_batch_device with no assumptions and a NULL carry_in, whose outputs
      must be equal;
  (b) effect of carrying: a first query under 3 random assumptions per formula leaves its
      lemmas in the regions (not timed); the second query, under 3 fresh random assumptions,
      is solved fresh (NULL carry_in, regions of its own) and carrying the first one's kept
      lemmas (carry_in = the first query's carry_out, in its regions).

One JSON line per repetition and a summary line with the medians, the answers and the
conflicts, rounds and carried lemmas per formula.  [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-mpi-stana-andrei_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from satmi import _capi, cdcl_sound, cnf  # noqa: E402

WARMUP = 2
B, N, M, SEED, ROOM, NASSUME = 4096, 50, 213, 4260, 1 << 14, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdcl_carry", "cdcl_carry_time.jsonl"))
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    batch = cnf.uniform_ksat(B, N, M, 3, seed=SEED)
    rng = np.random.default_rng(SEED)
    draw = lambda: (np.stack([rng.choice(N, NASSUME, replace=False) + 1 for _ in range(B)])   # noqa: E731
                    * rng.choice((-1, 1), (B, NASSUME))).reshape(-1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)   # noqa: E731
    first_lits, second_lits = up(draw()), up(draw())
    t = [up(a) for a in (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits, batch.inst_nvars)]
    regions = {k: z(B * ROOM) for k in ("fresh", "carried")}
    lb = torch.arange(B + 1, dtype=torch.int64, device=dev) * ROOM
    names = ("assume_none", "carry_none", "first", "second_fresh", "second_carried")
    outs = {k: dict(status=z(B), counters=z(B * 8, torch.int64), row_len=z(B), row_lits=z(B * N),
                    info=z(B * 4, torch.int64), core_len=z(B), core_lits=z(B * NASSUME), carry=z(B * 2, torch.int64))
            for k in names}
    none_begin, some_begin = z(B + 1), up(np.arange(B + 1) * NASSUME)
    s = torch.cuda.Stream(dev)

    def solve(name, region, begin, lits, carry_in=None, entry="carry"):
        o = outs[name]
        a = [B, *(x.data_ptr() for x in t), N, 3, regions[region].data_ptr(), lb.data_ptr(), o["status"].data_ptr(),
             o["counters"].data_ptr(), o["row_len"].data_ptr(), o["row_lits"].data_ptr(), N, o["info"].data_ptr(),
             begin.data_ptr(), lits.data_ptr(), o["core_len"].data_ptr(), o["core_lits"].data_ptr(), NASSUME]
        if entry == "assume":
            cdcl_sound.cdcl_assume_device(*a, stream=s.cuda_stream)
        else:
            cdcl_sound.cdcl_carry_device(*a, None if carry_in is None else carry_in.data_ptr(), o["carry"].data_ptr(),
                                         stream=s.cuda_stream)

    legs = (("assume_none_ms", lambda: solve("assume_none", "fresh", none_begin, first_lits, entry="assume")),
            ("carry_none_ms", lambda: solve("carry_none", "fresh", none_begin, first_lits)),
            ("second_fresh_ms", lambda: solve("second_fresh", "fresh", some_begin, second_lits)),
            ("second_carried_ms", lambda: solve("second_carried", "carried", some_begin, second_lits,
                                                outs["first"]["carry"])))
    times = {k: [] for k, _ in legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        with torch.cuda.stream(s):
            solve("first", "carried", some_begin, first_lits)     # its lemmas stay in the "carried" regions
            s.synchronize()
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
                    emit(dict(rep=rep - WARMUP, **row))
        host = {k: {n: v.cpu().numpy() for n, v in o.items()} for k, o in outs.items()}
        for n in ("status", "counters", "row_len", "row_lits", "info"):
            if not np.array_equal(host["assume_none"][n], host["carry_none"][n]):
                raise SystemExit(f"cdcl_carry_time: without a carry `{n}` differs from satmi_cdcl_assume_batch_device's")
        done = (_capi.CDCL_SOUND_SAT, _capi.CDCL_SOUND_UNSAT, _capi.CDCL_SOUND_ASSUMED)
        for k in names:
            if not np.isin(host[k]["status"], done).all():
                raise SystemExit(f"cdcl_carry_time: a search of `{k}` did not finish (a region too small?)")
        fresh, carried = host["second_fresh"], host["second_carried"]
        sat = lambda o: o["status"] == _capi.CDCL_SOUND_SAT   # noqa: E731
        if not np.array_equal(sat(fresh), sat(carried)):
            raise SystemExit("cdcl_carry_time: the carried second query's verdicts differ from the fresh one's")
        ctr = lambda k: host[k]["counters"].reshape(B, 8)   # noqa: E731
        summary = {"formulas": B, "max_vars": N, "max_clauses": M, "assumptions": NASSUME, "reps": args.reps,
                   "second_sat": int(sat(fresh).sum()), "second_refuted": int((~sat(fresh)).sum()),
                   "carried_lemmas_per_formula": float(host["first"]["carry"].reshape(B, 2)[:, 0].mean()),
                   "carried_words_per_formula": float(host["first"]["carry"].reshape(B, 2)[:, 1].mean()),
                   "first_conflicts_per_formula": float(ctr("first")[:, 0].mean())}
        for k in ("second_fresh", "second_carried", "carry_none"):
            summary[k + "_conflicts_per_formula"] = float(ctr(k)[:, 0].mean())
            summary[k + "_rounds_per_formula"] = float(ctr(k)[:, 3].mean())
        for k, v in times.items():
            summary.update({k + "_median": float(np.median(v)), k + "_min": min(v), k + "_max": max(v)})
        summary["carry_none_over_assume_none"] = summary["carry_none_ms_median"] / summary["assume_none_ms_median"]
        summary["second_carried_over_fresh"] = summary["second_carried_ms_median"] / summary["second_fresh_ms_median"]
        emit(summary)


if __name__ == "__main__":
    main()
