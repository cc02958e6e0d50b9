"""bench.py's printed line stays parseable: main()'s JSON assembly
(compact_line) on stub legs is under LINE_BUDGET bytes and keeps every key of
the driver's contract, the headline's full roofline / issue roofline / CPU
baseline, and each leg's figures (CPU only, no GPU).

The stubs are the r05 final line (profiles/r05/final/bench.json: 25 KB
uncompacted, the line the driver could not parse) with every leg of
bench.LEGS filled from its largest leg."""
import copy
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _full_line():
    with open(os.path.join(ROOT, "profiles", "r05", "final", "bench.json")) as fh:
        full = json.load(fh)
    biggest = max(full["configs"].values(), key=lambda r: len(json.dumps(r)))
    for name, _, _ in bench.LEGS:   # every leg this bench runs, each as large as the largest r05 leg
        full["configs"].setdefault(name, copy.deepcopy(biggest))
    return full


def test_compact_line_fits_the_budget():
    full = _full_line()
    assert len(json.dumps(full)) > bench.LINE_BUDGET   # the stub is a real oversized line
    line = json.dumps(bench.compact_line(full))
    assert len(line.encode()) < bench.LINE_BUDGET, len(line)
    assert "\n" not in line


def test_compact_line_keeps_the_contract_and_the_headline_figures():
    full = _full_line()
    c = bench.compact_line(full)
    for k in CONTRACT:
        assert k in c, k
    for k in ("value", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert c[k] == full[k], k   # the headline's own numbers unrounded
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in c["roofline"], k
    assert abs(c["roofline"]["frac"] / full["roofline"]["frac"] - 1) < 1e-3
    for k in ("bound", "frac", "fracs", "stale"):
        assert k in c["roofline_issue"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c["cpu_baseline"], k
    assert set(c["configs"]) == set(full["configs"])
    for name, leg in c["configs"].items():
        for k in ("value", "unit", "ms_per_step", "steps", "roofline", "cpu_baseline"):
            assert k in leg, (name, k)
        assert abs(leg["value"] / full["configs"][name]["value"] - 1) < 1e-3


def test_compact_line_without_legs_or_baseline():
    full = _full_line()
    for k in ("configs", "configs_note", "roofline_issue", "cpu_baseline", "branch_split"):
        full.pop(k, None)
    c = bench.compact_line(full)
    assert "configs" not in c and c.get("cpu_baseline") is None
    json.dumps(c)


def test_plain_run_measures_only_the_headline(monkeypatch, capsys):
    """Without --full no CPU baseline, oracle check or secondary config runs;
    --full brings all of them back, and its legs keep their CPU baselines."""
    plain = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert plain.steps == 3 and plain.warmup == 1 and not plain.full and plain.dump_outputs is None
    assert not bench.measures_cpu(plain) and not bench.measures_legs(plain, 1)
    for wl in ("3sat-n50", "php-dp", "php-res", "rand-dp", "cdcl"):
        assert not bench.measures_cpu(bench.parse(["--workload", wl]))
    full = bench.parse(["--full"])
    assert bench.measures_cpu(full) and bench.measures_legs(full, 1) and not bench.measures_legs(full, 2)
    assert not bench.measures_cpu(bench.parse(["--full", "--no-cpu-baseline"]))
    assert not bench.measures_legs(bench.parse(["--full", "--no-legs"]), 1)
    assert not bench.measures_legs(bench.parse(["--full", "--total", "4096"]), 1)
    assert not bench.measures_legs(bench.parse(["--full", "--workload", "uf250"]), 1)
    seen = []
    monkeypatch.setattr(bench, "run_one", lambda a, world, rank, local: seen.append(a) or {"value": 1.0})
    for hwq in ([], ["--legs-hwq17"]):
        bench.legs_main(bench.parse(["--legs-only"] + hwq))
        capsys.readouterr()
    assert len(seen) == len(bench.LEGS) and all(bench.measures_cpu(a) for a in seen)


def test_dump_outputs_keeps_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs: float arrays of the rows kept, every row while they fit,
    else the same seeded sample each time, the model zeroed past its length
    and the ticks counter left out."""
    import numpy as np
    import torch
    B, n = 1000, 10
    g = torch.Generator().manual_seed(5)
    status = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
    counters = torch.randint(0, 2**40, (B, 8), generator=g, dtype=torch.int64)
    sol_len = torch.randint(0, n + 1, (B,), generator=g, dtype=torch.int32)
    sol_lits = torch.randint(-n, n + 1, (B, n), generator=g, dtype=torch.int32)

    def dump(name, budget, suffix=""):
        d = tmp_path / name
        bench.dump_outputs(str(d), status, counters, sol_len, sol_lits, suffix, budget=budget)
        return d, {f.name[:-len(suffix + ".npy")]: np.load(f) for f in d.iterdir()}

    d, a = dump("all", bench.DUMP_BUDGET)
    assert set(a) == {"rows", "status", "counters", "sol_len", "sol_lits"}
    assert a["rows"].tolist() == list(range(B)) and a["counters"].shape == (B, 7) and a["sol_lits"].shape == (B, n)
    assert {k: v.dtype for k, v in a.items()} == {"rows": np.float64, "status": np.float32, "counters": np.float64,
                                                  "sol_len": np.float32, "sol_lits": np.float32}
    assert (a["counters"] == counters[:, :7].numpy()).all() and (a["status"] == status.numpy()).all()
    live = np.arange(n)[None, :] < sol_len.numpy()[:, None]
    assert (a["sol_lits"] == np.where(live, sol_lits.numpy(), 0)).all()

    budget = 5 * 4096 + 300 * (8 + 4 + 56 + 4 + 4 * n)
    d1, s1 = dump("sample1", budget)
    d2, s2 = dump("sample2", budget, suffix=".rank3")
    assert sum(f.stat().st_size for f in d1.iterdir()) <= budget
    rows = s1["rows"].astype(np.int64)
    assert len(rows) == 300 and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < B
    for k in a:
        assert (s1[k] == s2[k]).all(), k                       # the same sample every time
        assert (s1[k] == a[k][rows]).all(), k                  # ... of the same outputs
    assert sorted(f.name for f in d2.iterdir())[0] == "counters.rank3.npy"


def test_cpu_baseline_is_scaled_only_when_asked():
    """configs[2] / configs[1] time instances the oracle actually solves: the
    node-capped, scaled sample is the uf250-solved leg's alone (--cpu-scaled)."""
    assert not bench.parse([]).cpu_scaled
    assert not bench.parse(["--workload", "3sat-n50"]).cpu_scaled
    scaled = [name for name, _, extra in bench.LEGS if "--cpu-scaled" in extra]
    assert scaled and all("solved" in name for name in scaled)
