"""A plain bench.py run on the GPU (a small batch, one child process): --steps
sets the timed steps, the line carries the headline figures and nothing of
--full, and --dump-outputs writes what the last timed step returned -- checked
here against the step's own batch: every dumped model satisfies its formula
and a sample of instances equals the CPU oracle bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from satmi import _capi, cnf

pytestmark = pytest.mark.gpu
CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import torch
    total, steps, n, k = 8192, 3, 100, 3
    m = int(round(4.26 * n))
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--total", str(total), "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1                                   # one JSON result line
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "instances/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / total - 1) < 1e-9   # value = instances / step time
    assert line.get("cpu_baseline") is None and "configs" not in line          # those are --full's

    a = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(a) == {"rows", "status", "counters", "sol_len", "sol_lits"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
    assert a["rows"].tolist() == list(range(total))          # everything fits: no sampling
    sat = a["counters"][:, 5] > 0
    assert int(sat.sum()) == line["last_step_totals"]["sat"]
    assert int(a["counters"][:, 0].sum()) == line["last_step_totals"]["nodes"]
    assert ((a["status"] == _capi.DPLL_STOPPED) == sat).all()
    assert ((a["status"] == _capi.DPLL_STOPPED) | (a["status"] == _capi.DPLL_EXHAUSTED)).all()

    # the batch of the last timed step: step j runs resident batch j mod streams
    j = (steps - 1) % line["config"]["streams"]
    icb, clb, lits, nv = bench.chunked_batch(0, total, n, m, k, bench.batch_seed(bench.parse([]).seed, j),
                                             torch.device("cuda", 0))
    host = cnf.CnfBatch(icb.cpu().numpy(), clb.cpu().numpy(), lits.cpu().numpy(), nv.cpu().numpy())
    sol_len, sol_lits = a["sol_len"].astype(np.int64), a["sol_lits"].astype(np.int64)
    assert (sol_lits[np.arange(n)[None, :] >= sol_len[:, None]] == 0).all()
    val = np.zeros((total, n + 1), dtype=np.int8)
    np.put_along_axis(val, np.abs(sol_lits), np.sign(sol_lits).astype(np.int8), axis=1)
    val[:, 0] = 0
    lv = host.lits.reshape(total, m * k).astype(np.int64)
    litval = np.take_along_axis(val, np.abs(lv), axis=1) * np.sign(lv)
    clause_ok = (litval.reshape(total, m, k) > 0).any(axis=2).all(axis=1)
    assert (~sat | clause_ok).all()
    rng = np.random.default_rng(11)
    for b in list(rng.choice(np.flatnonzero(sat), 4, replace=False)) + list(rng.choice(np.flatnonzero(~sat), 4,
                                                                                       replace=False)):
        o = oracle.dpll(host.instance(int(b)), "sound", max_solutions=1, sol_cap=1)
        for c, key in enumerate(CTR):
            assert int(a["counters"][b, c]) == o["counters"][key], (int(b), key)
        if sat[b]:
            assert sol_lits[b, :sol_len[b]].tolist() == o["solutions"][0]
