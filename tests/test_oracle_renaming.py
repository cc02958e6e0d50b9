"""The CPU oracle's SOUND search is equivariant under an injective renaming of
variables, which is what lets test_dpll_gpu.py move one small exhaustive
search into every layout class of the clause kernels (tests/scan_cores.py);
and the guards of the 5-SAT threshold fixture that test reads."""
import hashlib
import json
import os

import pytest

import oracle
import scan_cores
from satmi import cnf

# per core: one UNSAT search and two SAT ones, the cheaper of each (the GPU
# test runs every instance of the core)
SAMPLE = {"A": (0, 8, 14), "B": (0, 2, 7), "C": (1, 2, 5)}


@pytest.mark.parametrize("core", sorted(SAMPLE))
def test_sound_search_is_equivariant_under_renaming(core):
    """Status, the six counters and the first model (element by element, in the
    assignment's insertion order) of a core instance renamed into 1..N equal
    those of the instance itself, mapped through the renaming -- for N at an
    8-bit / 16-bit code edge (255), inside the 16-bit class (300) and inside
    the 12-bit codes of the 5-slot word (1500).  The renaming puts a variable
    on N itself and one on 1."""
    fs = scan_cores.core_formulas(core)
    n = scan_cores.CORES[core][1]
    base = {b: oracle.dpll(fs[b], "sound", max_solutions=1, sol_cap=1) for b in SAMPLE[core]}
    assert {o["status"] for o in base.values()} == {0, 1}   # an exhausted tree and a model
    for N in (255, 300, 1500):
        img = scan_cores.renaming(core, N)
        assert len(img) == n + 1 and len(set(img[1:])) == n
        assert min(img[1:]) == 1 and max(img[1:]) == N
        for b, o in base.items():
            g = scan_cores.rename(fs[b], img)
            assert max(abs(l) for c in g for l in c) == N and min(abs(l) for c in g for l in c) == 1
            r = oracle.dpll(g, "sound", max_solutions=1, sol_cap=1)
            assert r["status"] == o["status"], (core, N, b)
            for k in scan_cores.CTR:
                assert r["counters"][k] == o["counters"][k], (core, N, b, k)
            assert r["solutions"] == scan_cores.rename(o["solutions"], img), (core, N, b)


def test_renaming_identity_and_ends():
    assert scan_cores.renaming("A", 40) == list(range(41))
    for core, N in (("A", 41), ("C", 127), ("C", 2047)):
        img = scan_cores.renaming(core, N)[1:]
        assert len(set(img)) == len(img) and 1 in img and N in img and all(1 <= v <= N for v in img)
    assert scan_cores.rename([[1, -2, 3]], [0, 7, 1, 9]) == [[7, -1, 9]]


def test_fullsolve_5sat50thr_fixture_guards(golden_dir):
    """tests/golden/fullsolve_5sat50thr.json (make_fullsolve.py): the instances
    regenerate bit-identically from the seed, all 16 searches are kept, 5 of
    them exhaust their tree, and the oracle reproduces the shortest one."""
    with open(os.path.join(golden_dir, "fullsolve_5sat50thr.json")) as fh:
        g = json.load(fh)
    assert (g["n"], g["m"], g["k"], g["seed"], g["count"]) == (50, 1056, 5, 5050, 16)
    batch = cnf.uniform_ksat(g["count"], g["n"], g["m"], g["k"], seed=g["seed"])
    assert hashlib.sha256(batch.lits.tobytes()).hexdigest() == g["lits_sha256"]
    cases = g["cases"]
    assert len(cases) == 16 >= 8
    assert sum(c["status"] == 0 for c in cases) >= 5
    c = min(cases, key=lambda c: c["counters"]["nodes"])
    o = oracle.dpll(batch.instance(c["index"]), "sound", max_solutions=1, sol_cap=1)
    assert o["status"] == c["status"] and o["counters"] == c["counters"]
    assert (o["solutions"][0] if o["solutions"] else []) == c["model"]
