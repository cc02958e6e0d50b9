"""CPU checks of the witness rule (tests/witness_rows.py's evaluator, which
tests/test_witness_gpu.py holds the kernel to): against brute force on seeded small
formulas, with records from the restatement of REF.py:63-130 in tests/witness_rows.py.
Half the formulas are clean; half have repeated literals and +v, -v in one clause."""
import random

import pytest

import witness_rows as wr

COUNT = 2100   # per kind: 4,200 formulas


@pytest.fixture(scope="module")
def runs():
    """(formula, has an empty clause, satisfiable, [(name, answer, record, stages, highest_only)])."""
    out = []
    rng = random.Random(5)
    for clean, seed in ((True, 11), (False, 12)):
        for f in wr.random_formulas(seed, COUNT, clean):
            ok_r, rec = wr.ref_resolution(f)
            ok_d, popped, lists = wr.ref_davis_putnam(f, rng if len(out) % 2 else None)
            flat = [c for group in lists for c in group]
            out.append((f, [] in f, wr.satisfiable(f),
                        [("resolution", ok_r, rec, wr.resolution_stages(f, rec) if ok_r else None, True),
                         ("davis-putnam", ok_d, flat, wr.elimination_stages(len(f), popped, lists) if ok_d else None,
                          False)]))
    return out


def test_every_true_on_a_formula_without_an_empty_clause_gives_a_model(runs):
    trues = {"resolution": 0, "davis-putnam": 0}
    for f, has_empty, sat, solvers in runs:
        for name, answer, record, stages, ho in solvers:
            if not answer or has_empty:
                continue
            trues[name] += 1
            words, n, row = wr.evaluate(f, record, stages, ho)
            assert words == [wr.MODEL, 0, -1, 0, 0, -1], (name, f, words)
            assert n == len(row) == len({abs(l) for c in f for l in c})
            assert wr.satisfies(f, row) and sat, (name, f, row)
    assert min(trues.values()) > 1000, trues


def test_model_always_means_the_row_satisfies_the_formula(runs):
    """Whatever the stages: the solver's own, the other solver's flag, shuffled, cut short."""
    rng = random.Random(7)
    models = others = 0
    for f, _, sat, solvers in runs[::3]:
        for name, answer, record, stages, ho in solvers:
            if not answer:
                continue
            bent = list(stages)
            rng.shuffle(bent)
            for st, flag in ((stages, ho), (stages, not ho), (bent, ho), (stages[1:], ho), ([], ho)):
                words, n, row = wr.evaluate(f, record, st, flag)
                holds = wr.satisfies(f, row)
                assert (words[0] == wr.MODEL) == holds == (words[4] == 0) == (words[5] == -1), (name, f, st, words)
                assert [abs(l) for l in row] == sorted({abs(l) for c in f for l in c})
                assert not holds or sat
                models += holds
                others += not holds
    assert models > 1000 and others > 100, (models, others)


def test_the_references_true_for_an_empty_clause_is_no_model():
    f = [[1], []]
    assert wr.ref_resolution(f) == (True, []) and wr.ref_davis_putnam(f) == (True, [1], [[[]]])
    want = [wr.NOT_MODEL, 0, -1, 0, 1, 1]
    assert wr.evaluate(f, [], wr.resolution_stages(f, []), True)[0] == want
    assert wr.evaluate(f, [[]], wr.elimination_stages(2, [1], [[[]]]), False)[0] == want
    assert not wr.satisfiable(f)


@pytest.mark.parametrize("case", range(len(wr.EDGE_CASES)))
def test_edge_cases_say_what_they_were_built_to_say(case):
    f, r, st, ho, words, row = wr.EDGE_CASES[case]
    assert wr.evaluate(f, r, st, ho) == (words, len(row), row)


def test_built_cases_are_models_only_through_their_decisive_parts():
    for n, at in wr.STAGE_SIZES:
        f, r, st, ho = wr.stage_size_case(n, at)
        assert wr.evaluate(f, r, st, ho)[0] == [wr.MODEL, 0, -1, 0, 0, -1]
        g = [c for i, c in enumerate(f) if i != at]
        assert wr.evaluate(g, r, [(1, 0, n - 1)], ho)[2] == [-1, -2]   # nothing else forces 1
    for k in wr.CLAUSE_LENGTHS:
        f, r, st, ho = wr.length_case(k)
        words, n, row = wr.evaluate(f, r, st, ho)
        assert words == [wr.MODEL, 0, -1, 0, 0, -1] and max(map(len, f)) == k
        assert row[:2] == ([1, -2] if k > 1 else [1])
    for v in wr.VARIABLE_IDS:
        f, r, st, ho = wr.variable_case(v)
        assert wr.evaluate(f, r, st, ho)[2] == [v - 1, v, -(v + 1)]
    fs, rs, ss = wr.forty()
    words, lens, rows = wr.expected(fs, rs, ss)
    assert all(w == [wr.MODEL, 0, -1, 0, 0, -1] for w in words) and lens == [3] * 40
    assert all((l > 0) == (i % 2 == 0) for i, row in enumerate(rows) for l in row)


def test_bad_literals_stages_and_truncation():
    f = [[1, 9], [-1, 0], [2, wr.I32_MIN]]
    words, n, row = wr.evaluate(f, [], [(1, 0, 3), (2, 0, 3), (0, 0, 3), (4, 0, 3), (-1, 0, 3)], False, max_vars=3)
    assert words == [wr.NOT_MODEL, 1, 0, wr.BAD_LITERAL | wr.BAD_STAGE, 1, 1] and row == [1, 2]
    # a bad literal in a record clause counts only when a stage reads the clause
    assert wr.evaluate([[1]], [[7]], [(1, 0, 1)], False, max_vars=3)[0][3] == 0
    assert wr.evaluate([[1]], [[7]], [(1, 0, 2)], False, max_vars=3)[0][3] == wr.BAD_LITERAL
    # under highest_only a bad literal is a magnitude: 9 > 1, INT32_MIN > anything, 0 < 1
    assert wr.evaluate([[1, 9]], [], [(1, 0, 1)], True, max_vars=3)[2] == [-1]
    assert wr.evaluate([[1, wr.I32_MIN]], [], [(1, 0, 1)], True, max_vars=3)[2] == [-1]
    assert wr.evaluate([[1, 0]], [], [(1, 0, 1)], True, max_vars=3)[2] == [1]
    g = [[1, 2, 3]]
    assert wr.evaluate(g, [], [], stride=3)[0][3] == 0
    words, n, row = wr.evaluate(g, [], [(3, 0, 1)], stride=2)
    assert (words[3], n, row) == (wr.ROW_TRUNCATED, 3, [-1, -2])
