"""CPU checks of the sound CDCL's rule under assumptions in Python (tests/cdcl_assume_rows.py):
without assumptions it is cdcl_sound_rows.solve; with them its three answers are held to brute
force, its cores to the assumptions, and its lemma lists to a plain RUP check against the
formula plus the core's unit clauses."""
import functools
import random

import cdcl_assume_rows as A
import cdcl_sound_rows as R


def _units(lits):
    return [[l] for l in lits]


def test_without_assumptions_it_is_the_sound_rule():
    for name, f in R.rows():
        w, g = R.solve(f), A.solve(f)
        assert {k: g[k] for k in w} == w, name
        assert g["core"] == ([] if w["status"] == R.UNSAT else None), name
    f = R.php(4)
    assert A.solve(f, (), conflict_limit=3)["lemmas"] == R.solve(f, conflict_limit=3)["lemmas"]


def test_rule_equals_brute_force_under_random_assumptions():
    rng = random.Random(0xA55)
    count = {A.SAT: 0, A.UNSAT: 0, A.ASSUMED: 0}
    strict = 0
    for f in R.random_small(0xCDC2, 3000):
        nv = max([abs(l) for c in f for l in c] + [1])
        assume = A.random_assumptions(rng, nv)
        r = A.solve(f, assume)
        count[r["status"]] += 1
        both = f + _units(assume)
        assert (r["status"] == A.SAT) == R.brute_force(both), (f, assume)
        if r["status"] == A.SAT:
            assert R.satisfies(both, r["model"]) and r["core"] is None
            assert [abs(l) for l in r["model"]] == sorted({abs(l) for c in both for l in c})
        elif r["status"] == A.UNSAT:
            assert not R.brute_force(f) and r["core"] == [] and A.refutes(f, r["lemmas"])
        else:
            core = r["core"]
            assert core and A.is_sublist(core, assume), (f, assume, core)
            assert not R.brute_force(f + _units(core)), (f, assume, core)
            assert A.refutes(f + _units(core), r["lemmas"]), (f, assume, core)
            assert all(A.rup(f + r["lemmas"][:j], c) for j, c in enumerate(r["lemmas"][:-1]))   # from F alone
            strict += len(set(core)) < len(set(assume))
        learned = [c for c in r["lemmas"] if c]
        c = dict(zip(A.COUNTERS, r["counters"]))
        assert c["learned"] == len(learned) and c["conflicts"] == len(learned) + (r["status"] == A.UNSAT)
        assert c["max_level"] <= len(assume) + c["decisions"]
    assert sum(count.values()) == 3000 and all(n >= 100 for n in count.values()), count
    assert strict >= 100, strict


@functools.lru_cache(maxsize=None)
def _row_results():
    return {name: (f, a, A.solve(f, a)) for name, f, a in A.rows()}


def test_rows_meet_their_conditions():
    by = _row_results()
    r = by["unit against its assumption"][2]
    assert (r["status"], r["core"], r["lemmas"]) == (A.ASSUMED, [-1], [[]])
    r = by["contradicting assumptions"][2]
    c = dict(zip(A.COUNTERS, r["counters"]))
    assert (r["status"], r["core"]) == (A.ASSUMED, [-3, 3]) and c["max_level"] == 2 and c["decisions"] == 0
    r = by["empty levels and a new variable"][2]
    assert (r["status"], r["model"]) == (A.SAT, [1, -2, 5])
    for n in (1, 2, 64, 65):
        r = by[f"chain of {n}"][2]
        assert r["status"] == A.ASSUMED and r["core"] == list(range(n, 0, -1)) and r["lemmas"] == [[]]
    f, a, r = by["php 3 under six selectors"]
    assert r["status"] == A.ASSUMED and sorted(r["core"]) == A.SELECTORS and len(r["lemmas"]) > 2
    assert A.refutes(f + _units(r["core"]), r["lemmas"])
    for drop in r["core"]:       # every selector is needed
        assert R.brute_force([c for c in f if -drop not in c])
    assert by["php 3 under five selectors"][2]["status"] == A.SAT
    f, a, r = by["unit lemma through two assumption levels"]
    c = dict(zip(A.COUNTERS, r["counters"]))
    assert r["status"] == A.SAT and [len(x) for x in r["lemmas"]] == [1] and c["max_level"] >= 3
    assert R.satisfies(f + _units(a), r["model"])


def test_random_row_has_every_answer():
    """Formula i has i % 4 assumptions over distinct variables; the unassumed quarter supplies
    the plain UNSAT answers."""
    got = []
    for i, (f, a) in enumerate(A.random_row()):
        assert len(a) == i % 4 and len({abs(l) for l in a}) == len(a)
        got.append(_row_results()[f"random 3-SAT {i} assumed"][2]["status"])
    assert len(got) == A.RANDOM_COUNT
    assert all(got.count(s) >= 4 for s in (A.SAT, A.UNSAT, A.ASSUMED)), got


def test_assumed_random_rows_are_refuted_with_their_cores():
    n = 0
    for name, (f, a, r) in _row_results().items():
        if r["status"] == A.ASSUMED:
            assert A.is_sublist(r["core"], a), name
            assert A.refutes(f + _units(r["core"]), r["lemmas"]), name
            n += 1
    assert n >= 10


def test_conflict_limit_under_assumptions():
    f, a = R.php(4), [1, 6, 11]      # three pigeons in three holes: the other two meet in the fourth
    r = A.solve(f, a, conflict_limit=1)
    assert r["status"] == A.LIMIT and r["counters"][0] == 1 and r["lemmas"] == [] and r["core"] is None
