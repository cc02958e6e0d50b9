"""The analysis half of a search node in the clause-scan kernels (dpll_scan.hip:
scan_counts, choose, first_flagged, first_of_pures): the byte-code class reads
the variables in one sweep, and writes the flags of the position scans only for
pure literals and for ties.

Every family drives one path of that code and compares the fixed kernel
(KERNEL_INC, dpll_fixed_kernel's shape class) with oracle.dpll(..., "sound")
bit for bit: status, nodes / decisions / unit_props / pure_assigns / conflicts /
solutions, sol_len and the model (assignment order, so a wrong branch variable
or a wrong pure-literal order shows); the rounds counter, which the oracle does
not keep, is pinned against the general kernel.  test_families_reach_their_paths
needs no GPU: _analysis() restates the reference's literal_sign / var_counts
pass on the root formula, and with the oracle's model shows that each family
reaches the path it is named after.
"""
import random

import pytest

import oracle
from satmi import _capi
from satmi.dpll import dpll_batch

gpu = pytest.mark.gpu

CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")

_oracle_cache = {}


def _oracle(name, fs):
    if name not in _oracle_cache:
        _oracle_cache[name] = [oracle.dpll(f, "sound", max_solutions=1, sol_cap=1) for f in fs]
    return _oracle_cache[name]


def _run(fs, policy):
    _capi.set_kernel(policy)
    _capi.set_split(_capi.SPLIT_OFF)
    try:
        return dpll_batch(fs, mode="sound", max_solutions=1, sol_cap=1)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
        _capi.set_split(True)


def _check(name, fs):
    n = max(abs(l) for f in fs for c in f for l in c)
    m = max(len(f) for f in fs)
    L = max(sum(len(c) for c in f) for f in fs)
    _capi.set_kernel(_capi.KERNEL_INC)
    try:
        kern, lds, _ = _capi.plan(n, m, L, 3)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    assert kern == _capi.KERNEL_INC and lds == 5108, "not dpll_fixed_kernel's shape class"
    want = _oracle(name, fs)
    r = _run(fs, _capi.KERNEL_INC)
    for b, o in enumerate(want):
        assert int(r.status[b]) == o["status"], (name, b)
        got = r.counter_dict(b)
        for key in CTR:
            assert got[key] == o["counters"][key], (name, b, key)
        model = o["solutions"][:1]
        assert r.solutions(b) == model, (name, b)
        if model:
            assert int(r.sol_len[b, 0]) == len(model[0]), (name, b)
    rg = _run(fs, _capi.KERNEL_GENERAL)   # rounds: the same count as the general kernel's
    assert (r.counters[:, :7] == rg.counters[:, :7]).all(), name


# ---- the reference's analysis of a formula with no unit clause (REF.py:174-208)

def _analysis(f, true_lits=()):
    """literal_sign / var_counts over the clauses `true_lits` leave active, in
    dict order (first positions): (pure variables, candidates of the largest
    count), both in dict order."""
    sign, count = {}, {}
    for c in f:
        if any(l in true_lits for l in c):
            continue
        for l in c:
            if -l in true_lits:
                continue
            sign.setdefault(abs(l), set()).add(l > 0)
            count[abs(l)] = count.get(abs(l), 0) + 1
    pures = [v for v in sign if len(sign[v]) == 1]
    top = max(count.values()) if count else 0
    return pures, [v for v in count if count[v] == top]


def _no_units(f):
    return all(len(c) >= 2 for c in f)


def _rand3(rng, n, m, force=()):
    f = [[v * rng.choice((1, -1)) for v in rng.sample(range(1, n + 1), 3)] for _ in range(m)]
    for i, c in force:
        f[i] = list(c)
    return f


# ---- the families: (formulas, a check of the formulas and the oracle's results that needs no GPU)

def _fam_ties(seed=201):
    """64 random 3-SAT instances, n=20, m=85, whose root analysis is a tie: no
    unit clause, no pure literal, several variables with the largest count."""
    rng = random.Random(seed)
    fs = []
    while len(fs) < 64:
        f = _rand3(rng, 20, 85)
        pures, cands = _analysis(f)
        if not pures and len(cands) > 1:
            fs.append(f)

    def check(want):
        later = 0
        for f, o in zip(fs, want):
            pures, cands = _analysis(f)
            assert _no_units(f) and not pures and len(cands) > 1
            assert o["root_assign"] == [] and o["counters"]["decisions"] >= 1
            if o["solutions"]:   # the first decision is the first candidate in dict order
                assert abs(o["solutions"][0][0]) == cands[0], f
            later += cands[0] != min(cands)
        assert later >= 16   # the dict-order winner is often not the lowest variable
        assert sum(bool(o["solutions"]) for o in want) >= 8 and sum(not o["solutions"] for o in want) >= 8
    return fs, check


def _fam_first_head_satisfied():
    """Variables 2 and 3 tie for the largest count once the root unit 1 is
    true; variable 2 comes first in the clause array, but in a clause that 1
    satisfies, so dict order over the active clauses picks 3."""
    f = [[1], [1, 2, 4], [3, 5, 6], [2, -3, 4], [-2, 3, -5], [-2, 4, -6], [2, 3, -4], [-2, -3, 7],
         [-4, 6, -7], [5, -6, -7]]
    fs = [f, [c[::-1] for c in f], f[:3] + f[:2:-1], [c[::-1] for c in f[:3] + f[:2:-1]]]

    def check(want):
        for f, o in zip(fs, want):
            assert o["root_assign"] == [1]
            pures, cands = _analysis(f, true_lits=(1,))
            assert not pures and sorted(cands) == [2, 3] and cands[0] == 3
            assert [abs(l) for c in f for l in c if len(c) > 1].index(2) < [abs(l) for c in f for l in c
                                                                           if len(c) > 1].index(3)
            assert o["solutions"] and abs(o["solutions"][0][1]) == 3, o
    return fs, check


def _fam_pures(seed=203):
    """Only pure literals (every variable occurs with one sign), and pure
    literals beside a tie of the other variables."""
    rng = random.Random(seed)
    only = []
    for n in (5, 20, 70):
        sg = {v: rng.choice((1, -1)) for v in range(1, n + 1)}
        only.append([[v * sg[v] for v in rng.sample(range(1, n + 1), 3)] for _ in range(3 * n)])
    beside = []
    while len(beside) < 13:
        f = _rand3(rng, 20, 60)
        pures, cands = _analysis(f)
        if pures and len(cands) > 1 and not set(pures) & set(cands):
            beside.append(f)
    fs = only + beside

    def check(want):
        for f, o in zip(fs[:3], want[:3]):
            pures, _ = _analysis(f)
            nv = len({abs(l) for c in f for l in c})
            assert len(pures) == nv and o["counters"]["pure_assigns"] == nv and o["counters"]["decisions"] == 0
            assert [abs(l) for l in o["solutions"][0]] == pures   # assigned in dict order
        for f, o in zip(fs[3:], want[3:]):
            pures, cands = _analysis(f)
            assert _no_units(f) and pures and len(cands) > 1
            assert o["counters"]["pure_assigns"] >= len(pures)
            if o["solutions"]:
                assert [abs(l) for l in o["solutions"][0][:len(pures)]] == pures
    return fs, check


def _fam_sweep_boundary(n, seed):
    """Every variable 1..n occurs (n = 64: one sweep step, full; 65: the second
    step holds one variable; 127: both full, byte codes' last variable)."""
    rng = random.Random(seed)
    m = min(448, int(round(4.26 * n)))
    fs = []
    while len(fs) < 16:
        f = _rand3(rng, n, m)
        if {abs(l) for c in f for l in c} == set(range(1, n + 1)):
            fs.append(f)
    # the largest count on the last variable alone, and tied between the first and the last
    for both in (False, True):
        f = [[v * rng.choice((1, -1)) for v in rng.sample(range(2, n), 3)] for _ in range(m)]
        for k, i in enumerate(range(0, m - 1, 8)):
            others = rng.sample(range(2, n), 2)
            f[i] = [n * (1 if k % 2 else -1), others[0], -others[1]]
            if both:
                f[i + 1] = [(1 if k % 2 else -1), -others[0], others[1]]
        fs.append(f)

    def check(want):
        assert all(max(abs(l) for c in f for l in c) == n and len(f) <= 448 for f in fs)
        _, c1 = _analysis(fs[-2])
        _, c2 = _analysis(fs[-1])
        assert c1 == [n] and sorted(c2) == [1, n]
        assert sum(o["counters"]["decisions"] > 0 for o in want) >= 16
    return fs, check


def _fam_long_list(seed=205):
    """n=10, m=120: a literal with 32 or more occurrences (the occurrence-list
    offsets of such an instance do not fit an offset-and-length word)."""
    rng = random.Random(seed)
    fs = []
    for lit in (1, -10, 5, -3):
        f = _rand3(rng, 10, 120)
        others = [v for v in range(1, 11) if v != abs(lit)]
        for i in rng.sample(range(120), 40):
            c = [lit] + [v * rng.choice((1, -1)) for v in rng.sample(others, 2)]
            rng.shuffle(c)
            f[i] = c
        fs.append(f)

    def check(want):
        for f in fs:
            lits = [l for c in f for l in set(c)]
            assert max(lits.count(l) for l in set(lits)) >= 32
            assert len(f) == 120 and max(abs(l) for c in f for l in c) == 10
    return fs, check


def _fam_many_candidates(seed=206):
    """n=100, m=70: every variable occurs exactly twice, once with each sign, in
    clauses of distinct variables (60 of three literals, 10 of two): no pure
    literal, and all 100 variables tie -- more candidates than a wave has lanes."""
    fs = []
    for s in range(4):
        rng = random.Random(seed + s)
        while True:
            slots = [v for v in range(1, 101)] + [-v for v in range(1, 101)]
            rng.shuffle(slots)
            sizes = [3] * 60 + [2] * 10
            rng.shuffle(sizes)
            f, at = [], 0
            for k in sizes:
                f.append(slots[at:at + k])
                at += k
            if all(len({abs(l) for l in c}) == len(c) for c in f):
                break
        fs.append(f)

    def check(want):
        for f, o in zip(fs, want):
            pures, cands = _analysis(f)
            assert len(f) == 70 and _no_units(f) and not pures and len(cands) == 100
            assert o["counters"]["decisions"] >= 1 and o["solutions"]
            assert abs(o["solutions"][0][0]) == abs(f[0][0])
    return fs, check


FAMILIES = {
    "ties": _fam_ties,
    "first-head-satisfied": _fam_first_head_satisfied,
    "pures": _fam_pures,
    "n64": lambda: _fam_sweep_boundary(64, 264),
    "n65": lambda: _fam_sweep_boundary(65, 265),
    "n127": lambda: _fam_sweep_boundary(127, 327),
    "long-list": _fam_long_list,
    "many-candidates": _fam_many_candidates,
}
_family_cache = {}


def _family(name):
    if name not in _family_cache:
        _family_cache[name] = FAMILIES[name]()
    return _family_cache[name]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_families_reach_their_paths(name):
    fs, check = _family(name)
    assert max(len(f) for f in fs) <= 448 and all(1 <= len(c) <= 3 for f in fs for c in f)
    assert max(abs(l) for f in fs for c in f for l in c) <= 127
    check(_oracle(name, fs))


@gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_analysis_parity(name):
    fs, _ = _family(name)
    _check(name, fs)
