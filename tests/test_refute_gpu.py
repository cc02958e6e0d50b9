"""GPU checks of the batched refutation check (csrc/refute.hip) through the C ABI:
every word of every instance and every lemma verdict against the plain Python
evaluator of tests/refute_rows.py (held to brute force by tests/test_refute.py).
Outputs are allocated with guard words on both sides, and the guards are asserted
intact.  The host form is run, and the device form at the true max_clause_len
(the lane-per-clause form up to 8) and at 0 (the wave-per-clause form)."""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import refute_rows as rr
from satmi import _capi
from satmi.check import check_models
from satmi.dp import eliminate, eliminate_batch
from satmi.refute import (check_refutations, check_refutations_device, debug_grid, proof_of_elimination,
                          proof_of_resolution)
from satmi.resolution import resolve, resolve_batch
from satmi.solvers import check_refutation

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
NG = 16   # guard words on each side


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _csr(lists):
    """Lists of clause lists -> (inst_begin, clause_begin, lits) int32, any literal kept as it is."""
    icb, clb, lits = [0], [0], []
    for f in lists:
        for c in f:
            lits += c
            clb.append(len(lits))
        icb.append(len(clb) - 1)
    return tuple(np.array(a or [0], dtype=np.int64).astype(np.int32) for a in (icb, clb, lits))


def _guarded(n):
    buf = np.full(2 * NG + n, GUARD, dtype=np.uint32).view(np.int32)
    return buf, buf[NG:NG + n]


def _intact(buf):
    g = np.asarray(buf).view(np.uint32)
    return (g[:NG] == GUARD).all() and (g[-NG:] == GUARD).all()


def run_host(formulas, proofs):
    """satmi_check_refutations_host into guarded outputs -> ([B][4] words, the lemma verdicts)."""
    B, P = len(formulas), sum(map(len, proofs))
    f, p = _csr(formulas), _csr(proofs)
    obuf, out = _guarded(B * 4)
    kbuf, ok = _guarded(P)
    rc = _capi.load().satmi_check_refutations_host(B, *map(_p, f), *map(_p, p), _p(out), _p(ok))
    _capi.check(rc, "satmi_check_refutations_host")
    assert _intact(obuf) and _intact(kbuf)
    return out.reshape(B, 4).tolist(), ok.tolist()


def run_device(formulas, proofs, max_vars, max_clause_len, lemmas=True):
    """satmi_check_refutations_device on torch tensors, guarded outputs."""
    import torch
    dev = torch.device("cuda", 0)
    B, P = len(formulas), sum(map(len, proofs))
    t = [torch.from_numpy(a).to(dev) for a in _csr(formulas) + _csr(proofs)]
    obuf = torch.full((2 * NG + B * 4,), GUARD, dtype=torch.int32, device=dev)
    kbuf = torch.full((2 * NG + P,), GUARD, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    check_refutations_device(B, *(x.data_ptr() for x in t), max_vars, max_clause_len, obuf.data_ptr() + 4 * NG,
                             kbuf.data_ptr() + 4 * NG if lemmas else None, s.cuda_stream)
    s.synchronize()
    ho, hk = obuf.cpu().numpy(), kbuf.cpu().numpy()
    assert _intact(ho) and _intact(hk)
    if not lemmas:
        assert (hk.view(np.uint32) == GUARD).all()
    return ho[NG:-NG].reshape(B, 4).tolist(), hk[NG:NG + P].tolist()


def _true_max_len(formulas, proofs):
    return max([len(c) for f in formulas + proofs for c in f] + [0])


def check_all(formulas, proofs, want=None):
    """Host form and both device forms against the evaluator (`want`: what it said before);
    returns the expected pair."""
    want = want or rr.expected(formulas, proofs)
    assert run_host(formulas, proofs) == want
    mv = max([rr.max_vars_of(f, p) for f, p in zip(formulas, proofs)] + [0])
    for mcl in (_true_max_len(formulas, proofs), 0):
        assert run_device(formulas, proofs, mv, mcl) == want, mcl
    return want


# ------------------------------------------------------------------ 1. the edge batch, in one launch
def test_edge_batch_in_one_launch():
    fs, ps = [c[0] for c in rr.EDGE_CASES], [c[1] for c in rr.EDGE_CASES]
    words, oks = check_all(fs, ps)
    assert words == [c[2] for c in rr.EDGE_CASES]
    assert oks == [v for c in rr.EDGE_CASES for v in c[3]]
    # d_lemma_ok = NULL: the same words, nothing written
    assert run_device(fs, ps, 4, 3, lemmas=False)[0] == words
    res = check_refutations(fs, ps, lemmas=True)
    assert [[r[k] for k in _capi.REFUTE_WORDS] for r in res] == words
    assert [r["proven"] for r in res] == [w[0] == rr.PROVEN for w in words]
    assert [r["lemma_ok"] for r in res] == [c[3] for c in rr.EDGE_CASES]
    assert "lemma_ok" not in check_refutations(fs, ps)[0]
    assert check_refutation([[1], [-1]], [[]])
    assert not check_refutation(rr.QUAD + [[-1]], [[]])            # implied, but no unit propagation gets there
    assert check_refutation(rr.QUAD + [[-1]], [[2], []])
    assert not check_refutation([[1], [-1]], [[2]])                # every lemma verified, the empty clause not reached


# ------------------------------------------------------------------ 2. propagation depth
@pytest.mark.parametrize("k", rr.DEPTHS)
def test_propagation_depth(k):
    cases = rr.chain_cases(k)
    words, oks = check_all([f for f, _ in cases], [p for _, p in cases])
    assert oks == [1, 1 if k == 1 else 0, 1]


# ------------------------------------------------------------------ 3. same-step collisions
def test_two_clauses_of_one_step_force_both_signs():
    """[-1, 2] and [-1, -2] sit in the same 64-clause step; under the lemma [-1] they force +2
    and -2 at once, with no clause that is falsified under either: the conflict is the atomic's."""
    f = [[-1, 2], [-1, -2]]
    words, oks = check_all([f, f + [[3, 4]] * 61 + [[-1, 5], [-1, -5]]], [[[-1]], [[-1], [-3]]])
    assert oks == [1, 1, 0]


def test_sixty_four_copies_of_one_unit_push_one_trail_entry():
    """max_vars = 1: the trail has room for one entry, and under the empty lemma the 64 lanes
    of a step all find the unit [1] (the empty lemma fails: nothing conflicts).  The lemma
    checked next on the wave is the next instance's, over the same variable with the other
    sign: a bit left in the table would be its conflict, or its tautology."""
    f, g = [[1]] * 64, [[-1]] * 64
    fs, ps = [f, g, f, g, f], [[[]]] * 4 + [[[-1], [1]]]
    try:
        for grid in ((1, 1), (1, 2), (1, 4), (0, 0)):
            debug_grid(*grid)
            words, oks = check_all(fs, ps)
            assert oks == [0, 0, 0, 0, 0, 1] and [w[3] for w in words] == [0] * 5
    finally:
        debug_grid(0, 0)


# ------------------------------------------------------------------ 4. state between lemmas and instances
def test_assumptions_do_not_survive_a_lemma():
    """[3] verifies through a check that assigns -3, 1 and 2 and falsifies [-2, 3]; the lemma
    after it is unrelated ([4]) or satisfies what was assigned ([-2]) and must fail: with any
    of those bits left over, [-2, 3] or [3, 1] would be its conflict."""
    f = [[3, 1], [-1, 2], [-2, 3]]
    words, oks = check_all([f, f], [[[3], [4]], [[3], [-2]]])
    assert oks == [1, 0, 1, 0] and words == [[rr.FAILED, 1, 1, 0]] * 2


def _forty():
    fs, ps = [], []
    for i in range(40):
        f, p = rr.random_small(100 + i, count=1, nmax=5)[0] if i % 4 else rr.EDGE_CASES[i % 16][:2]
        fs.append(f)
        ps.append(p)
    return fs, ps


@pytest.mark.parametrize("grid", [(1, 1), (1, 2), (1, 4), (3, 2), (3, 4), (0, 0)])
def test_forty_instances_under_every_grid(grid):
    """(1, 1): one wave takes all 40, so a bit that survived an instance shows in the next;
    2- and 4-wave workgroups: the regions do not overlap."""
    fs, ps = _forty()
    try:
        debug_grid(*grid)
        words, _ = check_all(fs, ps)
        assert len({w[0] for w in words}) == 3
    finally:
        debug_grid(0, 0)


# ------------------------------------------------------------------ 5. counts
def test_clause_counts_with_the_decisive_clause_last():
    cases = [rr.clause_count_case(m) for m in rr.CLAUSE_COUNTS]
    words, oks = check_all([f for f, _ in cases], [p for _, p in cases])
    assert oks == [0, 1, 1, 1, 1, 1]


def test_lemma_counts_where_a_lemma_needs_the_one_before_it():
    cases = [rr.lemma_count_case(k) for k in rr.LEMMA_COUNTS]
    words, _ = check_all([f for f, _ in cases], [p for _, p in cases])
    assert words == [[rr.OPEN, 0, -1, 0]] + [[rr.FAILED, k - 1, 0, 0] for k in rr.LEMMA_COUNTS[1:]]


# ------------------------------------------------------------------ 6. clause lengths, both forms
@pytest.mark.parametrize("k", rr.CLAUSE_LENGTHS)
def test_clause_lengths_in_both_forms(k):
    """k = 8 is the last length of the lane-per-clause form, 9 the first of the
    wave-per-clause form; max_clause_len = 0 (unknown) takes the latter at every length."""
    cases = rr.length_case(k)
    words, oks = check_all([f for f, _ in cases], [p for _, p in cases])
    assert (words, oks) == ([[rr.OPEN, 0, -1, 0], [rr.FAILED, 1, 0, 0]], [1, 0, 1])


def test_mixed_clause_lengths_in_one_instance():
    """Every length in one instance (the true max_clause_len is 300: the long form), and the
    lengths up to 8 in one (the short form), their variables renumbered apart."""
    for lengths in (rr.CLAUSE_LENGTHS, tuple(range(1, rr.SHORT_MAX + 1))):
        f, p, base = [], [], 0
        for k in lengths:
            for fk, pk in rr.length_case(k):
                f += [[l + base if l > 0 else l - base for l in c] for c in fk]
                p += [[l + base if l > 0 else l - base for l in c] for c in pk]
                base += k + 2
        words, oks = check_all([f], [p])
        assert oks == [1, 0, 1] * len(lengths)


# ------------------------------------------------------------------ 7. variable range
def test_variable_range():
    top = rr.MAX_VARS
    f = [[-top, 1], [top, 1], [-1, top - 1], [-1, 1 - top]]
    p = [[1], [], [top]]
    words, oks = check_all([f, f[:3]], [p, p])
    assert oks == [1, 1, -1, 1, 0, -1]
    g = [[1, top + 1]]
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        check_refutations([g], [[[1]]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        run_device([f], [p], top + 1, 2)
    # sparse ids
    f = [[30000, 3], [-30000, 3], [-3, 29999], [-3, -29999]]
    words, oks = check_all([f], [[[3], []]])
    assert (words, oks) == ([[rr.PROVEN, 0, -1, 0]], [1, 1])


def test_bad_literals_through_the_device_form():
    """max_vars = 3 where the arrays hold 9, 0 and INT32_MIN: a formula clause that holds one is
    no premise, a lemma that holds one fails and is no premise; both set the flag."""
    fs = [[[1, 9], [-1]], [[1], [-1]], [[1]], [[1]], [[1], [-1]], [[2, 0], [-2, rr.I32_MIN], [1]]]
    ps = [[[]], [[9], []], [[0, 1]], [[rr.I32_MIN, 2, -2]], [[], [9]], [[3], [1]]]
    want = rr.expected(fs, ps, 3)
    assert want[0] == [[rr.FAILED, 1, 0, 2], [rr.FAILED, 1, 0, 2], [rr.FAILED, 1, 0, 2], [rr.FAILED, 1, 0, 3],
                       [rr.PROVEN, 0, -1, 0], [rr.FAILED, 1, 0, 2]]
    assert want[1] == [0, 0, 1, 0, 0, 1, -1, 0, 1]
    for mcl in (3, 0):
        assert run_device(fs, ps, 3, mcl) == want, mcl


# ------------------------------------------------------------------ 8. the solvers' own records
RES_SEED, DP_SEED = 2, 2   # both verdicts among the 32 formulas (asserted against the oracle below)


@pytest.fixture(scope="module")
def records():
    """name -> (formulas, the batched solver's dicts, their proofs, what the evaluator says of them)."""
    out = {}
    for name, n, m, seed, solve, build in (("resolution", 6, 40, RES_SEED, resolve_batch, proof_of_resolution),
                                           ("elimination", 8, 48, DP_SEED, eliminate_batch, proof_of_elimination)):
        fs = rr.random_3sat(32, n, m, seed)
        rs = solve(fs, record=True)
        ps = [build(r) for r in rs]
        out[name] = (fs, rs, ps, rr.expected(fs, ps))
    return out


@pytest.mark.parametrize("name", ["resolution", "elimination"])
def test_recorded_proofs_verify(records, name):
    fs, rs, ps, want = records[name]
    verdicts = [r["result"] for r in rs]
    ref = oracle.resolution if name == "resolution" else oracle.dp
    assert verdicts == [ref(f)["result"] for f in fs]
    assert 0 in verdicts and 1 in verdicts and set(verdicts) == {0, 1}
    assert all((p[-1:] == [[]]) == (v == 0) and [] not in p[:-1] for p, v in zip(ps, verdicts))
    words, oks = check_all(fs, ps, want)
    assert words == [[rr.PROVEN if v == 0 else rr.OPEN, 0, -1, 0] for v in verdicts]
    assert oks == [1] * len(oks)   # every derived clause verifies
    res = check_refutations(fs, ps)
    assert [r["proven"] for r in res] == [v == 0 for v in verdicts]


@pytest.mark.parametrize("name", ["resolution", "elimination"])
def test_recorded_proofs_with_one_literal_negated(records, name):
    fs, _, ps, _ = records[name]
    rng = random.Random(11)
    bent = [rr.negate_one(p, rng) or p for p in ps]
    assert sum(a != b for a, b in zip(bent, ps)) >= 30
    words, _ = check_all(fs, bent)
    assert any(w[0] == rr.FAILED for w in words)


def test_single_formula_records():
    for f, solve, build, ref in ((rr.random_3sat(1, 6, 40, 5)[0], resolve, proof_of_resolution, oracle.resolution),
                                 (rr.random_3sat(1, 8, 48, 5)[0], eliminate, proof_of_elimination, oracle.dp)):
        r = solve(f, record=True)
        assert r["result"] == ref(f)["result"] and r["result"] in (0, 1)
        p = build(r)
        words, oks = check_all([f], [p])
        assert words == [[rr.PROVEN if r["result"] == 0 else rr.OPEN, 0, -1, 0]] and oks == [1] * len(p)
        assert check_refutation(f, p) == (r["result"] == 0)
        assert len(p) > 1
        check_all([f], [rr.negate_one(p, random.Random(3))])


# ------------------------------------------------------------------ 9. the reference's unsound refutation
def test_the_references_unsound_refutation_fails():
    """resolution_solver resolves {1, -1} with {-1} on literal 1 into the empty clause and
    answers False for a formula that x1 = False satisfies."""
    f = [[1, -1], [-1]]
    r = resolve(f, record=True)
    assert oracle.resolution(f)["result"] == 0 and r["result"] == 0
    p = proof_of_resolution(r)
    assert p == [[]]   # the first pass ends in the empty resolvent: nothing is recorded before it
    words, oks = check_all([f], [p])
    assert words == [[rr.FAILED, 1, 0, 0]] and oks == [0]
    assert not check_refutation(f, p)
    assert check_models([f], [[[-1]]])[0][0]["ok"]


# ------------------------------------------------------------------ 10. four host threads
def test_four_host_threads(records):
    fs, _, ps, want = records["elimination"]
    cuts = [0, 5, 14, 23, 32]

    def part(t):
        a, b = cuts[t], cuts[t + 1]
        return run_host(fs[a:b], ps[a:b])

    with ThreadPoolExecutor(4) as ex:
        for _ in range(3):
            parts = list(ex.map(part, range(4)))
            assert sum((w for w, _ in parts), []) == want[0]
            assert sum((k for _, k in parts), []) == want[1]
