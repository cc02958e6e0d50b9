"""Record tests/golden/dpll_plan_table.json: what one build of the library
answers to the queries of tests/dpll_plan_rows.py (the general DPLL kernel's
two layouts, the clause kernels' eligibility layout, the choice of kernel).
No query makes a HIP call, so this runs without a GPU.

The table is a record of the build a change starts from, not of the build it
ends with: build the parent commit's library with the same hipcc line into
satmi/libsatmi_parent.so and run

    SATMI_LIB_VARIANT=libsatmi_parent.so python tests/golden/make_golden_plan.py

tests/test_dpll_plan_table.py then holds the new build to it.  Re-record only
when a change means to move a layout or the choice, and say so.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sat-mpi-stana-andrei_amd")]

import dpll_plan_rows  # noqa: E402
from satmi import _capi  # noqa: E402

OUT = os.path.join(HERE, "dpll_plan_table.json")


def main():
    L = _capi.load()
    rows = [dict(q, answer=dpll_plan_rows.ask(L, q)) for q in dpll_plan_rows.queries(L)]
    with open(OUT, "w") as fh:
        fh.write('{"meta": %s,\n "rows": [\n' % json.dumps({"generator": "tests/golden/make_golden_plan.py"}))
        fh.write(",\n".join("  " + json.dumps(r) for r in rows))
        fh.write("\n ]}\n")
    by = {}
    for r in rows:
        by[r["fn"]] = by.get(r["fn"], 0) + 1
    print(OUT, os.path.basename(_capi.LIB_PATH), by)


if __name__ == "__main__":
    main()
