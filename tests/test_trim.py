"""CPU checks of the refutation trim's rule: the plain Python trimmer of
tests/trim_rows.py, which walks backwards and tracks reasons, is held to brute
force on every refute_rows.random_small pair (seeds 0-4) as it is and with []
appended, under three propagation orders; the rows that claim a unique answer
are shown to have it under those orders; and the Python wrappers' arguments."""
import pytest

import refute_rows as rr
import trim_rows as tr


@pytest.mark.parametrize("seed", range(5))
def test_python_trimmer_against_brute_force(seed):
    """PROVEN => the forward evaluator accepts (core, kept) with 0 failed, and the core alone is
    unsatisfiable by enumeration; forward PROVEN => PROVEN; FAILED => forward FAILED; no empty
    lemma => OPEN with no marks (all inside check_properties)."""
    proven = strict = 0
    for f, p in tr.random_rows([seed]):
        nvars = max(rr.max_vars_of(f, p), 1)
        for rng in tr.rng_orders():
            words, core, lemma = tr.trim(f, p, rng=rng)
            tr.check_properties(f, p, words, core, lemma, brute_nvars=nvars)
        if words[0] == rr.PROVEN and [] in p:
            proven += 1
            strict += sum(core) < len(f)
    assert proven > 50 and strict > 40   # the rows do reach PROVEN, mostly with a strict subset as the core


def test_rows_with_a_unique_answer():
    for f, p, status, core_idx, kept_idx in tr.unique_rows():
        for rng in tr.rng_orders():
            words, core, lemma = tr.trim(f, p, rng=rng)
            tr.check_properties(f, p, words, core, lemma)
            assert words[0] == status
            assert [c for c, x in enumerate(core) if x] == core_idx, (f[:6], p[:6])
            assert [j for j, x in enumerate(lemma) if x >= 0] == kept_idx


def test_reuse_rows_have_a_unique_answer():
    for f, p, core_idx, kept_idx in (tr.REUSE_A, tr.REUSE_B, tr.REUSE_D):
        for rng in tr.rng_orders():
            words, core, lemma = tr.trim(f, p, rng=rng)
            assert words[0] == rr.PROVEN
            assert [c for c, x in enumerate(core) if x] == core_idx
            assert [j for j, x in enumerate(lemma) if x >= 0] == kept_idx


def test_forward_failed_trim_proven_example():
    f, p = tr.XOR2 + [[3, 4]], [[5, 6], [2], []]
    assert rr.evaluate(f, p)[0][:3] == [rr.FAILED, 1, 0]
    words, core, lemma = tr.trim(f, p)
    assert words == [rr.PROVEN, 0, -1, 0, 4, 2] and core == [1, 1, 1, 1, 0] and lemma == [-1, 1, 1]


def test_count_and_length_rows_reach_the_empty_lemma():
    rows = tr.counts_rows() + [r for k in rr.CLAUSE_LENGTHS for r in tr.length_rows(k)]
    for f, p in rows:
        assert p[-1] == [] and [] not in p[:-1]
        for rng in tr.rng_orders():
            tr.check_properties(f, p, *tr.trim(f, p, rng=rng))
    # needed lemmas that fail: the chain of unforced implications, all marked from [k] or from []
    f, p = tr.lemma_chain_through_failed(65)
    for rng in tr.rng_orders():
        words, core, lemma = tr.trim(f, p, rng=rng)
        assert words[:3] == [rr.FAILED, 64, 0] and lemma[:64] == [0] * 64 and lemma[65] == 1


def test_bad_literals_and_tautologies_in_the_python_trimmer():
    """An unneeded bad lemma changes nothing; a needed one fails.  A tautological lemma is never
    needed: as a premise it is satisfied or has two open literals, so it is no reason and no
    conflict, and the ending lemma is empty -- it stays -1 and the flag stays 0 where the forward
    check sets it."""
    assert tr.trim([[1], [-1]], [[9], []], 3) == ([rr.PROVEN, 0, -1, 0, 2, 1], [1, 1], [-1, 1])
    words, core, lemma = tr.trim([[-9, 1], [-1]], [[1], []], 3)     # [1] is needed, and only the bad clause gives it
    assert (words, core, lemma) == ([rr.FAILED, 1, 0, rr.BAD_LITERAL, 1, 2], [0, 1], [0, 1])
    words, core, lemma = tr.trim([[1]], [[2, 9], [-1]], 3)          # no empty lemma
    assert (words, core, lemma) == ([rr.OPEN, 0, -1, 0, 0, 0], [0], [-1, -1])
    words, core, lemma = tr.trim([[1]], [[-1, 9], []], 3)           # the bad lemma would be what [] needs
    assert (words, core, lemma) == ([rr.FAILED, 1, 1, 0, 0, 1], [0], [-1, 0])
    f, p = [[1], [-1]], [[2, -2], []]
    assert rr.evaluate(f, p)[0] == [rr.PROVEN, 0, -1, rr.TAUTOLOGY]
    assert tr.trim(f, p) == ([rr.PROVEN, 0, -1, 0, 2, 1], [1, 1], [-1, 1])


def test_python_wrapper_arguments():
    from satmi.refute import trim_refutations
    with pytest.raises(ValueError, match="one list of lemmas per formula"):
        trim_refutations([[[1]]], [])
    with pytest.raises(ValueError, match="literal 0"):
        trim_refutations([[[1]]], [[[0]]])
    assert trim_refutations([], []) == []
