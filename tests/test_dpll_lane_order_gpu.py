"""Unit rounds ranked by lane order (dpll_scan.hip, inc_units): the occurrence
lists are ascending in clause index, so the unit scan of a batch of ONE literal
holds the touched clauses in clause order by lane, and its units are ranked
and assigned in the scan itself -- no bitmap, no snapshot, no assignment loop.

Every family builds rounds of that kind -- a root unit, or a decision, whose
negation's list makes N two-literal clauses unit at once -- and compares the
kernel with oracle.dpll(..., "sound") bit for bit: status, every counter the
oracle keeps, sol_len and the model (which is in assignment order, so a wrong
rank shows), unsplit and with SPLIT_ALWAYS at warm-up 0; unsplit, the rounds
counter is pinned against the general kernel.  _capi.plan confirms the kernel
class.  test_families_reach_their_paths needs no GPU: the formulas and the
oracle alone show that each family produces the round it is named after.

Construction (_round_formula): x = 1 is the literal assigned alone; target
clause i is [-x, lits[i]], shuffled; the targets sit at clause indices that
straddle the 32-clause words of the unit bitmap and the 64-clause blocks of the
list fill, among filler clauses -- most hold +x (satisfied with the targets'
round), a few are free 3-literal clauses over the auxiliary variables.  Slots
are shuffled and the y variables are numbered at random against clause order,
so a list kept in fill order (slot by slot within a block) ranks wrongly."""
import random

import pytest

import oracle
from satmi import _capi
from satmi.dpll import dpll_batch

gpu = pytest.mark.gpu

CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")
SPLITS = [_capi.SPLIT_OFF, _capi.SPLIT_ALWAYS]
X = 1
SIZES = (3, 8, 33, 64)

_oracle_cache = {}


def _oracle(name, fs):
    """The oracle's results of a family, computed once and shared by its cases."""
    if name not in _oracle_cache:
        _oracle_cache[name] = [oracle.dpll(f, "sound", max_solutions=1, sol_cap=1, paths=True) for f in fs]
    return _oracle_cache[name]


def _run(fs, policy, split):
    _capi.set_kernel(policy)
    _capi.set_split(split)
    _capi.set_split_warmup(0)
    try:
        return dpll_batch(fs, mode="sound", max_solutions=1, sol_cap=1)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
        _capi.set_split(True)
        _capi.set_split_warmup(-1)


def _check(name, fs, split, fixed=True):
    n = max(abs(l) for f in fs for c in f for l in c)
    m = max(len(f) for f in fs)
    L = max(sum(len(c) for c in f) for f in fs)
    k = max(len(c) for f in fs for c in f)
    assert all(len(c) >= 1 for f in fs for c in f)
    _capi.set_kernel(_capi.KERNEL_INC)
    try:
        kern, lds, _ = _capi.plan(n, m, L, k)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    assert kern == _capi.KERNEL_INC
    if fixed:
        assert lds == 5108, "not dpll_fixed_kernel's shape class"
    else:
        assert lds != 5108 and (n > 127 or k > 3), "not dpll_scan_kernel's shape class"
    want = _oracle(name, fs)
    r = _run(fs, _capi.KERNEL_INC, split)
    for b, o in enumerate(want):
        assert int(r.status[b]) == o["status"], (name, b)
        got = r.counter_dict(b)
        for key in CTR:
            assert got[key] == o["counters"][key], (name, b, key)
        model = o["solutions"][:1]
        assert r.solutions(b) == model, (name, b)
        if model:
            assert int(r.sol_len[b, 0]) == len(model[0]), (name, b)
    if split == _capi.SPLIT_OFF:   # rounds: one search per wave, the same count as the general kernel's
        rg = _run(fs, _capi.KERNEL_GENERAL, _capi.SPLIT_OFF)
        assert (r.counters[:, :7] == rg.counters[:, :7]).all(), name


# ---- the construction

def _indices(rng, N, m):
    """N clause indices below m: the word and block boundaries first, the rest at random."""
    base = [i for i in (31, 32, 64, 63, 65, 127, 128, 95, 96, 0) if i < m][:N]
    rest = rng.sample([i for i in range(m) if i not in base], N - len(base))
    return sorted(base + rest)


def _round_formula(rng, lits, mode, naux=8, ternary=0, m_min=200, targets=None, prefix=()):
    """See the module docstring.  mode "unit": the clause [x] makes x a root
    unit; "decision": no unit clause and no pure literal, and x occurs most, so
    x = True is the first decision.  `ternary`: further clauses [-x, a, b] of
    the same list that stay open.  `targets`: the target clauses themselves, if
    not [-x, lit].  `prefix`: clauses kept first, in order (a root chain)."""
    nvar = max([X] + [abs(l) for l in lits] + [abs(l) for c in prefix for l in c])
    aux = list(range(nvar + 1, nvar + 1 + naux))
    flip = {}

    def a(v=None):   # signs alternate per variable: both polarities occur
        v = rng.choice(aux) if v is None else v
        flip[v] = -flip.get(v, -1)
        return v * flip[v]

    tg = [list(c) for c in targets] if targets is not None else [[-X, l] for l in lits]
    for _ in range(ternary):
        p, q = rng.sample(aux, 2)
        tg.append([-X, a(p), a(q)])
    if ternary:
        rng.shuffle(tg)
    for c in tg:
        rng.shuffle(c)
    fill = []
    for _ in range(2 * naux):   # free clauses: what is left once x and the units are assigned
        fill.append([a(v) for v in rng.sample(aux, 3)])
    while len(tg) + len(fill) + len(prefix) + 1 < m_min:
        p, q = rng.sample(aux, 2)
        c = [X, a(p), a(q)]
        rng.shuffle(c)
        fill.append(c)
    pos = {l for c in tg + fill for l in c}
    for v in sorted({abs(l) for l in pos} - {X}):   # no pure literal: the missing polarity, beside +x
        for s in (v, -v):
            if s not in pos:
                c = [X, s, a()]
                rng.shuffle(c)
                fill.append(c)
    if mode == "unit" and not prefix:
        fill.append([X])
    rng.shuffle(fill)
    m = len(tg) + len(fill)
    at = set(_indices(rng, len(tg), m))
    ti, fi = iter(tg), iter(fill)
    return [list(c) for c in prefix] + [next(ti) if i in at else next(fi) for i in range(m)]


def _neg_list(f, x=X):
    """Clause indices of the occurrence list of -x (a clause once)."""
    return [i for i, c in enumerate(f) if -x in c]


def _fill_order_wrong(f, x=X):
    """Two clauses of -x's list in one 64-clause block, the lower one holding -x
    in a later slot: a list filled slot by slot would put the higher one first."""
    ix = _neg_list(f, x)
    return any(i // 64 == j // 64 and f[i].index(-x) > f[j].index(-x) for i in ix for j in ix if i < j)


def _straddles(f, x=X):
    ix = _neg_list(f, x)
    return len({i // 32 for i in ix}) >= 2 and len({i // 64 for i in ix}) >= 2


def _round_units(f, x=X):
    """REF.py:143's snapshot once x alone is true: the unit clauses in clause order."""
    out = []
    for c in f:
        if x in c:
            continue
        rest = [l for l in c if l != -x]
        if len(rest) == 1 and len(rest) < len(c):
            out.append(rest[0])
    return out


def _first_wins(units):
    """REF.py:146-164 on a snapshot: the assignments made, and whether it stopped
    in a conflict -- at the first entry whose negation is a unit clause too
    (the assignment empties that clause, REF.py:161-162)."""
    a = {}
    for l in units:
        if abs(l) in a:
            continue
        a[abs(l)] = l
        if -l in units:
            return list(a.values()), True
    return list(a.values()), False


def _no_unit_no_pure_x_most(f):
    lits = [l for c in f for l in c]
    cnt = {}
    for l in lits:
        cnt[abs(l)] = cnt.get(abs(l), 0) + 1
    return (all(len(c) >= 2 for c in f) and all(-l in lits for l in lits)
            and all(cnt[X] > k for v, k in cnt.items() if v != X))


def _ys(rng, N, mode):
    """N signed literals over variables 2..: distinct (64: 33 variables, so some twice), or with
    one variable two times and another three times, with the same or the opposite sign."""
    nv = min(N, 33)
    if mode != "distinct":
        nv = max(2, nv - (1 if N < 8 else 3))
    vs = list(range(2, 2 + nv))
    rng.shuffle(vs)
    lits = list(vs)
    if mode == "distinct":
        lits += [rng.choice(vs) for _ in range(N - nv)]
    else:
        s = -1 if mode == "opposite" else 1
        lits += [s * vs[0]] if N < 8 else [s * vs[0], s * vs[1], vs[1]]
        lits += [rng.choice(vs[2:]) for _ in range(N - len(lits))]
    rng.shuffle(lits)
    return lits


# ---- the families: (formulas, a check of the oracle's results that needs no GPU)

def _fam_rounds(entry, ymode, seed, sizes=SIZES + (65,), naux=8, m_min=None):
    rng = random.Random(seed)
    fs, metas = [], []
    for N in sizes:
        for _ in range(2):
            lits = _ys(rng, N, ymode)
            f = _round_formula(rng, lits, entry, naux=naux, m_min=m_min or (200 if N < 64 else 320))
            fs.append(f)
            metas.append((N, lits))

    def check(want):
        assert any(_fill_order_wrong(f) for f in fs)
        for f, (N, lits), o in zip(fs, metas, want):
            c, p = o["counters"], o["paths"]
            units = _round_units(f)
            assert len(_neg_list(f)) == N and _straddles(f)
            assert [abs(l) for l in units] == [abs(l) for l in lits] and len(units) == N
            got, stopped = _first_wins(units)
            assert stopped == (ymode == "opposite")
            if entry == "unit":
                assert [cl for cl in f if len(cl) == 1] == [[X]]
                assert o["root_assign"][:1 + len(got)] == [X] + got, (N, ymode)
            else:
                assert _no_unit_no_pure_x_most(f) and o["root_assign"] == [] and c["decisions"] >= 1
            assert p["snapshot_len_max"] >= N
            if ymode == "same":
                assert p["snapshot_same_var_same_sign"] >= 1 and len(got) < N
            if ymode == "opposite":
                assert c["conflicts"] >= 1
                if entry == "unit":   # the root stops at the mismatch: x and the entries assigned before it
                    assert o["status"] == _capi.DPLL_EXHAUSTED and c["conflicts"] == 1
                    assert c["unit_props"] == 1 + len(got), (N, c, len(got))
            else:
                assert o["solutions"] and o["solutions"][0][:1 + len(got)] == [X] + got, (N, ymode)
    return fs, check


def _fam_empty_with_units(seed):
    """Root chain q; then x and -x in one snapshot, either first: the literal of
    x's variable that is assigned makes N units and the other one's clause
    empty in the same scan.  That scan ends in inc_units()'s empty-clause
    return, before the lane-order branch: the family pins the cut of a
    one-entry batch over an ascending list, not the stamps the new branch
    writes (the *-opposite families cut through those, one round later)."""
    rng = random.Random(seed)
    fs, metas = [], []
    for N in (3, 8, 33):
        for xfirst in (True, False):
            lits = _ys(rng, N, "distinct")
            q = max(lits) + 1
            f = _round_formula(rng, lits, "unit", m_min=120, prefix=[[q]])
            two = [[-q, X], [-X, -q]] if xfirst else [[-X, -q], [-q, X]]
            cut = rng.randint(1, len(f) - 1)
            fs.append(f[:cut] + two[:1] + f[cut:] + two[1:])
            metas.append((N, xfirst, q))

    def check(want):
        for f, (N, xfirst, q), o in zip(fs, metas, want):
            c = o["counters"]
            assert f[0] == [q] and sum(len(cl) == 1 for cl in f) == 1
            assert o["status"] == _capi.DPLL_EXHAUSTED and c["conflicts"] == 1 and c["decisions"] == 0
            assert c["unit_props"] == 2 and o["root_assign"][:2] == [f[0][0], X if xfirst else -X]
            # with x true: N units beside the emptied clause [-x, -q]
            assert len(_round_units(f)) == N + 1 and -q in _round_units(f)
    return fs, check


def _fam_list_lengths(seed):
    """33 units in a list of 64 entries (one step) and of 65 (the general path)."""
    rng = random.Random(seed)
    fs, metas = [], []
    for T in (64, 65):
        for entry in ("unit", "decision"):
            lits = _ys(rng, 33, "distinct")
            fs.append(_round_formula(rng, lits, entry, ternary=T - 33, m_min=320))
            metas.append((T, entry, lits))

    def check(want):
        for f, (T, entry, lits), o in zip(fs, metas, want):
            units = _round_units(f)
            assert len(_neg_list(f)) == T and sorted(units) == sorted(lits) and _straddles(f)
            assert o["paths"]["snapshot_len_max"] >= 33
            if entry == "unit":
                assert o["root_assign"][:34] == [X] + units
            else:
                assert _no_unit_no_pure_x_most(f) and o["counters"]["decisions"] >= 1
    return fs, check


def _fam_repeats(seed):
    """Targets that repeat -x or the unit literal, and tautologies: one list entry each."""
    rng = random.Random(seed)
    fs = []
    for _ in range(4):
        ys = list(range(2, 14))
        rng.shuffle(ys)
        tg = []
        for i, y in enumerate(ys):
            tg.append([[-X, -X, y], [-X, y, -X], [y, -X, -X], [-X, y, y], [-X, X, y], [-X, y, -y]][i % 6])
        tg = [tg[i] for i in rng.sample(range(12), 12)]
        keep = [list(c) for c in tg]
        f = _round_formula(rng, ys, "unit", m_min=150, targets=tg)
        assert sorted(map(sorted, keep)) == sorted(sorted(c) for c in f if -X in c)
        fs.append(f)

    def check(want):
        for f, o in zip(fs, want):
            units = _round_units(f)
            assert len(_neg_list(f)) == 12 and len(units) == 6   # [-x, -x, y] in each slot order, twice
            assert o["root_assign"][:7] == [X] + units
    return fs, check


def _fam_random(seed, count=200):
    rng = random.Random(seed)
    fs = []
    for _ in range(count):
        n = rng.randint(10, 30)
        m = int(round(rng.uniform(4.0, 4.6) * n))
        fs.append([[v * rng.choice((1, -1)) for v in rng.sample(range(1, n + 1), 3)] for _ in range(m)])

    def check(want):
        assert sum(o["counters"]["decisions"] > 0 for o in want) >= 0.9 * count
        assert sum(o["counters"]["conflicts"] > 0 for o in want) >= 0.5 * count
        assert sum(bool(o["solutions"]) for o in want) >= 0.2 * count
        assert sum(not o["solutions"] for o in want) >= 0.2 * count
    return fs, check


FAMILIES = {
    "unit-distinct": lambda: _fam_rounds("unit", "distinct", 101),
    "decision-distinct": lambda: _fam_rounds("decision", "distinct", 102),
    "unit-same": lambda: _fam_rounds("unit", "same", 103, SIZES),
    "decision-same": lambda: _fam_rounds("decision", "same", 104, SIZES),
    "unit-opposite": lambda: _fam_rounds("unit", "opposite", 105, SIZES),
    "decision-opposite": lambda: _fam_rounds("decision", "opposite", 106, SIZES),
    "empty-with-units": lambda: _fam_empty_with_units(107),
    "list-lengths": lambda: _fam_list_lengths(108),
    "repeats": lambda: _fam_repeats(109),
    "random": lambda: _fam_random(110),
}
# dpll_scan_kernel's class (16-bit codes: more than 127 variables), through the same rounds
SCAN_FAMILIES = {
    "scan-unit-same": lambda: _fam_rounds("unit", "same", 111, SIZES, naux=100, m_min=400),
    "scan-decision-opposite": lambda: _fam_rounds("decision", "opposite", 112, SIZES, naux=100, m_min=400),
}
_family_cache = {}


def _family(name):
    if name not in _family_cache:
        _family_cache[name] = {**FAMILIES, **SCAN_FAMILIES}[name]()
    return _family_cache[name]


@pytest.mark.parametrize("name", list(FAMILIES) + list(SCAN_FAMILIES))
def test_families_reach_their_paths(name):
    fs, check = _family(name)
    n = max(abs(l) for f in fs for c in f for l in c)
    assert max(len(f) for f in fs) <= 448 and all(len(c) <= 3 for f in fs for c in f)
    assert 127 < n <= 140 if name in SCAN_FAMILIES else n <= 45
    check(_oracle(name, fs))


@gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_lane_order_parity(name, split):
    fs, _ = _family(name)
    _check(name, fs, split)


@gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", list(SCAN_FAMILIES))
def test_lane_order_parity_scan_class(name, split):
    fs, _ = _family(name)
    _check(name, fs, split, fixed=False)
