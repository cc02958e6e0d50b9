"""CPU checks of the sound CDCL's rule in Python (tests/cdcl_sound_rows.py): its verdict
against brute force and against the oracle's sound DPLL, its models against the formula, its
lemma lists against the refutation check's evaluator, and the rows' own conditions."""
import functools

import oracle
import cdcl_sound_rows as R
import refute_rows as rr


def _certified(formula, r, want_sat):
    assert r["status"] == (R.SAT if want_sat else R.UNSAT)
    if want_sat:
        assert R.satisfies(formula, r["model"])
        assert [abs(l) for l in r["model"]] == sorted({abs(l) for c in formula for l in c})
        assert all(c for c in r["lemmas"])            # no empty clause was learned
    else:
        assert r["model"] is None and r["lemmas"][-1] == []
        words, ok = rr.evaluate(formula, r["lemmas"])
        assert words[:3] == [rr.PROVEN, 0, -1] and all(x == 1 for x in ok)
    c = dict(zip(R.COUNTERS, r["counters"]))
    learned = [l for l in r["lemmas"] if l]
    assert c["learned"] == len(learned) and c["learned_literals"] == sum(map(len, learned))
    assert c["conflicts"] == c["learned"] + (0 if want_sat else 1) and c["restarts"] == 0
    assert all(len({abs(l) for l in lem}) == len(lem) for lem in learned)


def test_rule_equals_brute_force_on_small_formulas():
    formulas = R.random_small(0xCDC1, 3000)
    sat = 0
    for f in formulas:
        want = R.brute_force(f)
        sat += want
        _certified(f, R.solve(f), want)
    assert 500 < sat < 2500      # both verdicts are well represented


@functools.lru_cache(maxsize=None)
def _row_results():
    return [(name, f, R.solve(f)) for name, f in R.rows()]


def test_rows_equal_the_oracle_and_are_certified():
    """(A formula that holds the empty clause is unsatisfiable, but sound DPLL, like the
    reference's DPLL, never looks at an empty clause of its input and answers from the rest:
    for the one such row the verdict is held to brute force, and the oracle to its quirk.)"""
    for name, f, r in _row_results():
        o = oracle.dpll(f, "sound", max_solutions=1, sol_cap=1)
        assert o["status"] in (0, 1), name
        if [] in f:
            assert o["counters"]["solutions"] > 0 and not R.brute_force(f), name
            _certified(f, r, False)
        else:
            _certified(f, r, o["counters"]["solutions"] > 0)


def test_random_row_has_both_verdicts():
    got = [r["status"] for name, _, r in _row_results() if name.startswith("random 3-SAT")]
    assert len(got) == R.RANDOM_COUNT
    assert got.count(R.SAT) >= 8 and got.count(R.UNSAT) >= 8


def test_rows_meet_their_conditions():
    by = {name: (f, r) for name, f, r in _row_results()}
    assert by["empty formula"][1]["status"] == R.SAT and by["empty formula"][1]["model"] == []
    assert by["empty clause"][1]["lemmas"] == [[]] and by["opposite units"][1]["lemmas"] == [[]]
    # QUAD + [-1]: unit propagation alone does not refute it
    f, r = by["quad needs learning"]
    assert rr.evaluate(f, [[]])[0][0] == rr.FAILED and r["counters"][4] >= 1
    assert len(by["first learned clause is a unit"][1]["lemmas"][0]) == 1
    for k in (2, 8, 9, 64, 65):
        assert len(by[f"learned clause of {k}"][1]["lemmas"][0]) == k
    for m in (63, 64, 65, 129):
        assert len(by[f"{m} clauses"][0]) == m
    assert max(map(len, by["long clause"][0])) == 300
    assert max(abs(l) for c in by["sparse ids"][0] for l in c) == R.MAX_VARS
    assert by["sparse ids"][1]["status"] == R.UNSAT and by["sparse ids"][1]["counters"][4] >= 1
    for holes in (3, 4):
        assert by[f"php {holes}"][1]["status"] == R.UNSAT
    assert by["tautology only"][1]["model"] == [-4]


def test_conflict_limit_and_record_words():
    f = R.php(4)
    full = R.solve(f)
    assert full["counters"][0] > 3
    cut = R.solve(f, conflict_limit=3)
    assert cut["status"] == R.LIMIT and cut["counters"][0] == 3 and cut["lemmas"] == full["lemmas"][:2]
    assert R.region_words([[1, 2], []]) == 4
