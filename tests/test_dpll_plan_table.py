"""CPU: the built library answers the layout and kernel-choice queries of
tests/dpll_plan_rows.py exactly as the recorded table says
(tests/golden/dpll_plan_table.json, tests/golden/make_golden_plan.py).  None of
the queries makes a HIP call, so the table reads the same with and without a GPU."""
import json
import os

import dpll_plan_rows
from satmi import _capi


def _table(golden_dir):
    with open(os.path.join(golden_dir, "dpll_plan_table.json")) as fh:
        return json.load(fh)["rows"]


def test_library_reproduces_the_recorded_table(golden_dir):
    L = _capi.load()
    rows = _table(golden_dir)
    for row in rows:
        q = {k: v for k, v in row.items() if k != "answer"}
        got = dpll_plan_rows.ask(L, q)
        print(q, got)
        assert got == row["answer"], q


def test_table_has_both_sides_of_every_edge(golden_dir):
    """The record itself: every query of the module is in it, no plan row
    answers with a clause kernel (that answer needs the runtime), and each bound
    has a row that passes and a row that fails."""
    L = _capi.load()
    rows = _table(golden_dir)
    assert [{k: v for k, v in r.items() if k != "answer"} for r in rows] == dpll_plan_rows.queries(L)
    plans = [r for r in rows if r["fn"] == "plan"]
    assert {r["answer"]["kernel"] for r in plans} == {0, _capi.KERNEL_GENERAL, _capi.KERNEL_WIDE}
    assert {r["answer"]["rc"] for r in plans} == {0, -3}   # SATMI_OK, SATMI_ERR_TOO_LARGE
    for fn in ("lds_bytes", "scan_lds_bytes"):
        got = [r["answer"]["bytes"] for r in rows if r["fn"] == fn]
        # (the clause kernels' image grows by a 64-clause chunk of 8-byte words at a time)
        assert 0 in got and 160 * 1024 - 512 <= max(got) <= 160 * 1024
    wide = [r["answer"] for r in plans if r["answer"]["kernel"] == _capi.KERNEL_WIDE]
    assert all(a == {"rc": 0, "kernel": _capi.KERNEL_WIDE, "lds_bytes_per_wave": 256, "waves_per_cu": 32} for a in wide)
    # the LDS form from one resident wave per CU (a workgroup's LDS past 64 KiB) to all 32
    assert {r["answer"]["waves_per_cu"] for r in plans if r["answer"]["kernel"] == _capi.KERNEL_GENERAL} >= {1, 2, 32}
