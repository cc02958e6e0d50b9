"""CPU checks of the refutation check's rule: the plain Python evaluator of
tests/refute_rows.py (what tests/test_refute_gpu.py holds the kernel to) against
brute force, the hand cases pinned, and the proof builders of satmi/refute.py."""
import random

import pytest

import refute_rows as rr
from satmi.refute import proof_of_elimination, proof_of_resolution


def test_verified_lemmas_are_implied_by_brute_force():
    """On every generated formula of at most 5 variables: a verified lemma is implied by the
    formula and the lemmas before it (truth-table enumeration), the words are consistent with
    the lemma verdicts, and checking stops behind the first empty lemma."""
    verified = failed = 0
    for seed in (1, 2):
        for f, p in rr.random_small(seed):
            n = max(rr.max_vars_of(f, p), 1)
            assert n <= 5
            words, ok = rr.evaluate(f, p)
            stop = next((i for i, c in enumerate(p) if not c), len(p) - 1)
            assert ok[stop + 1:] == [-1] * (len(p) - stop - 1) and -1 not in ok[:stop + 1]
            for i in range(min(stop + 1, len(p))):
                if ok[i] == 1:
                    assert rr.implied(f + p[:i], p[i], n), (f, p, i)
                    verified += 1
                else:
                    failed += 1
            checked = ok[:stop + 1]
            assert words[1] == checked.count(0)
            assert words[2] == (checked.index(0) if 0 in checked else -1)
            ended = bool(p) and stop < len(p) and not p[stop]
            assert words[0] == (rr.FAILED if words[1] else rr.PROVEN if ended else rr.OPEN)
            assert bool(words[3] & rr.TAUTOLOGY) == any(-l in c for c in p[:stop + 1] for l in c)
            assert not words[3] & rr.BAD_LITERAL
    assert verified > 500 and failed > 200   # (incompleteness is pinned by hand: test_hand_cases)


def test_evaluator_is_order_independent():
    """Reaching a conflict does not depend on the order the premises are scanned in."""
    rng = random.Random(7)
    for f, p in rr.random_small(3, count=150):
        want = rr.evaluate(f, p)
        g = list(f)
        rng.shuffle(g)
        g = [rng.sample(c, len(c)) for c in g]
        assert rr.evaluate(g, p) == want


def test_hand_cases():
    for f, p, words, ok in rr.EDGE_CASES:
        assert rr.evaluate(f, p) == (words, ok), (f, p)
    # implied but not verified, and the proof that gets there
    assert rr.implied(rr.QUAD, [1], 3)
    assert rr.evaluate(rr.QUAD, [[1]])[1] == [0]
    assert rr.evaluate(rr.QUAD, [[1, 2], [1]])[1] == [1, 1]


def test_generated_cases_are_what_their_docstrings_say():
    for k in rr.DEPTHS:
        full, cut, forward = rr.chain_cases(k)
        assert rr.evaluate(*full)[1] == [1]
        assert rr.evaluate(*cut)[1] == [1 if k == 1 else 0]
        assert rr.evaluate(*forward)[1] == [1]
        assert rr.evaluate(forward[0][1:], forward[1])[1] == [0]
    for m in rr.CLAUSE_COUNTS:
        f, p = rr.clause_count_case(m)
        assert len(f) == m and rr.evaluate(f, p)[1] == [1 if m else 0]
        assert rr.evaluate(f[:-1], p)[1] == [0]
    for k in rr.LEMMA_COUNTS:
        f, p = rr.lemma_count_case(k)
        assert len(p) == k and rr.evaluate(f, p)[1] == [0] * (k - 1) + [1]
        if k > 1:   # without the lemma just before it the last one fails
            assert rr.evaluate(f, p[:-2] + p[-1:])[1][-1] == 0
    for k in rr.CLAUSE_LENGTHS:
        (fa, pa), (fb, pb) = rr.length_case(k)
        assert max(map(len, fa)) == max(k, 2) and all(len(c) == k for c in pa + pb)
        assert rr.evaluate(fa, pa) == ([rr.OPEN, 0, -1, 0], [1])
        assert rr.evaluate(fb, pb) == ([rr.FAILED, 1, 0, 0], [0, 1])


def test_bad_literals():
    """A premise with a bad literal is skipped, a lemma with one fails; both set the flag."""
    f = [[1, 9], [-1]]
    assert rr.evaluate(f, [[]], max_vars=3) == ([rr.FAILED, 1, 0, rr.BAD_LITERAL], [0])   # [1, 9] is no premise
    assert rr.evaluate(f, [[9]], max_vars=9) == ([rr.OPEN, 0, -1, 0], [1])
    assert rr.evaluate([[1], [-1]], [[9], []], max_vars=3) == ([rr.FAILED, 1, 0, rr.BAD_LITERAL], [0, 1])
    assert rr.evaluate([[1]], [[0, 1]], max_vars=3)[0] == [rr.FAILED, 1, 0, rr.BAD_LITERAL]
    assert rr.evaluate([[1]], [[rr.I32_MIN, 2, -2]], max_vars=3)[0] == [rr.FAILED, 1, 0, 3]
    assert rr.evaluate([[1], [-1]], [[], [9]], max_vars=3) == ([rr.PROVEN, 0, -1, 0], [1, -1])   # not checked


def test_proof_builders():
    res = {"result": 0, "passes": 2, "clauses": [[[1, 2], [3]], [[-3]]]}
    assert proof_of_resolution(res) == [[1, 2], [3], [-3], []]
    assert proof_of_resolution(dict(res, result=1)) == [[1, 2], [3], [-3]]
    assert proof_of_resolution(dict(res, result=-1)) == [[1, 2], [3], [-3]]
    dp = {"result": 0, "steps": 1, "vars": [1], "clauses": []}
    assert proof_of_elimination(dp) == [[]]
    assert proof_of_elimination({"result": 1, "clauses": [[[2, 3]], []]}) == [[2, 3]]
    for build in (proof_of_resolution, proof_of_elimination):
        with pytest.raises(ValueError, match="record"):
            build({"result": 0, "passes": 1})
