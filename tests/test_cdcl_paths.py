"""CPU: the rows of tests/cdcl_paths.py reach the paths of csrc/cdcl.hip they
claim, by the oracle's path counters (oracle/cdcl_oracle.c oracle_cdcl_paths),
and together they reach every one.  Conditions on the inputs only: the GPU
side (test_cdcl_paths_gpu.py) runs the same rows against the same oracle."""
import ctypes
import json
import operator
import os
import random

import pytest

import cdcl_paths
import oracle
from cdcl_paths import CDCL_PATH_ROWS, EQ, GE, PATH_REACHED, PATHS_NEVER

OPS = {GE: operator.ge, EQ: operator.eq}


def test_paths_entry_runs_the_same_search():
    """oracle_cdcl_paths is oracle_cdcl plus counters: same verdict, model, var_inc and counts."""
    for name, build, cap, _ in CDCL_PATH_ROWS[:6] + CDCL_PATH_ROWS[-1:]:
        plain = oracle.cdcl(cdcl_paths.row_formula(name), cap)
        withp = dict(cdcl_paths.row_oracle(name))
        assert set(withp.pop("paths")) == set(oracle.CDCL_PATHS)
        assert withp == plain, name


@pytest.mark.parametrize("row", CDCL_PATH_ROWS, ids=[r[0] for r in CDCL_PATH_ROWS])
def test_row_reaches_its_paths(row):
    name, _, _, needs = row
    paths = cdcl_paths.row_oracle(name)["paths"]
    print(name, {k: v for k, v in paths.items() if v not in (0, -1)})
    assert needs
    for counter, op, value in needs:
        assert OPS[op](paths[counter], value), f"{name}: {counter} = {paths[counter]}, needs {op} {value}"
    for counter in PATHS_NEVER:
        assert paths[counter] == 0, f"{name}: {counter} = {paths[counter]}"


def test_rows_cover_every_path():
    """Every counter of the oracle is either reached by a row -- required there
    at PATH_REACHED's value or beyond -- or listed as never moved: a counter
    (a path of the kernel) added without a row fails here."""
    assert set(PATH_REACHED) | set(PATHS_NEVER) == set(oracle.CDCL_PATHS)
    assert not set(PATH_REACHED) & set(PATHS_NEVER)
    for counter, reached in PATH_REACHED.items():
        rows = [name for name, _, _, needs in CDCL_PATH_ROWS
                if any(c == counter and v >= reached for c, _, v in needs)]
        assert rows, f"no row is required to reach {counter} >= {reached}"
    # both sides of the boundaries the kernel switches at
    def values(counter):
        return {v for _, _, _, needs in CDCL_PATH_ROWS for c, op, v in needs if c == counter and op == EQ}
    assert {63, 64, 65, 130} <= values("conflict_len_max") | values("learned_len_max")   # activity bump, 3 chunks
    assert {0, 63, 64, 129} <= values("maxlevel_pos_max")   # first / last of a chunk, the next chunk's first
    assert 8192 in values("table_slots_max") and 262144 in values("table_slots_max")
    assert len({name for name, _, _, _ in CDCL_PATH_ROWS}) == len(CDCL_PATH_ROWS)


def _random_batches():
    """The formulas of test_cdcl_gpu.py::test_cdcl_matches_oracle_random (same generator, same seeds)."""
    for seed, count, nmax, kmax, cap in [(1, 200, 16, 4, 3000), (2, 64, 40, 6, 20000)]:
        rng = random.Random(seed)
        for _ in range(count):
            n = rng.randint(2, nmax)
            f = []
            for _ in range(rng.randint(1, 5 * n)):
                k = rng.randint(1, min(kmax, n))
                c = [v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), k)]
                if rng.random() < 0.1:
                    c.append(c[0] if rng.random() < 0.5 else -c[0])
                f.append(c)
            yield f, cap


def test_antecedent_resolution_is_never_taken(golden_dir):
    """analyze_conflict's resolution loop (REF.py:331-342): only the unit clauses
    of the input set an antecedent, their variables sit at level 0, and the
    first maximal-level literal of a conflict on several levels is a decision.
    0 steps over the rows (test_row_reaches_its_paths), every golden case and
    the random batches of test_cdcl_gpu.py; nor is a unit clause ever learned."""
    with open(os.path.join(golden_dir, "cdcl_ref.json")) as fh:
        cases = [(c["formula"], c["max_iter"]) for c in json.load(fh)["cases"]]
    assert len(cases) > 100
    conflicts = 0
    for f, cap in cases + list(_random_batches()):
        o = oracle.cdcl(f, cap, paths=True)
        conflicts += o["stats"]["conflicts"]
        for counter in PATHS_NEVER:
            assert o["paths"][counter] == 0, (counter, f)
    assert conflicts > 100000   # the searches did analyse conflicts


def test_stale_library_is_rebuilt_or_refused(tmp_path):
    """oracle.lib() binds oracle_cdcl_paths: a library kept from a tree without
    that entry is rebuilt once, and refused if the rebuild does not bring it."""
    import subprocess
    assert hasattr(oracle.lib(), "oracle_cdcl_paths")
    src = os.path.dirname(os.path.abspath(oracle.__file__))
    cc = os.environ.get("CC", "gcc")
    stale = tmp_path / "stale.c"
    stale.write_text("int oracle_cdcl(void) { return 0; }\n")
    so = str(tmp_path / "liboracle.so")

    def compile_to(sources):
        subprocess.run([cc, "-O1", "-fPIC", "-shared", "-o", so] + sources, check=True)

    compile_to([str(stale)])
    with pytest.raises(RuntimeError, match="oracle_cdcl_paths"):
        oracle._open(so, rebuild=lambda: None)
    real = [os.path.join(src, n) for n in sorted(os.listdir(src)) if n.endswith(".c")]
    L = oracle._open(so, rebuild=lambda: compile_to(real))
    assert hasattr(L, "oracle_cdcl_paths")
    # a caller whose counter list is not the library's is refused too
    L.oracle_cdcl_paths.restype = ctypes.c_int
    assert L.oracle_cdcl_paths(0, None, None, ctypes.c_int64(1), None, None, None, None, None, 1) == -3
