"""The bench kernel's propagation rounds (dpll_scan.hip, dpll_fixed_kernel: K = 3,
n <= 127, m <= 448) against the CPU oracle, bit for bit: the decision literal
assigned by its caller (assign_decision, propagate's `dec` entry), and the
incremental unit scan over the occurrence lists on clauses that are legal
but unusual (repeats, tautologies, padding), with the propagated literal in
every slot, and at the batch sizes where the scan changes path.

Every family runs under the INC policy in the fixed kernel's shape class
(_capi.plan confirms it), unsplit and with SPLIT_ALWAYS at warm-up 0, and is
compared with oracle.dpll(..., "sound"): status, every counter the oracle
keeps (all but the GPU's rounds and ticks), sol_len and the model.  Unsplit,
the rounds counter (which the oracle does not keep) is pinned against the
general kernel.  Each family asserts from the oracle's counters, or from the
formula itself, that it produces the path it is named after.

Not constructible, so not covered: a *decision* whose literal's negation has an
empty occurrence list.  A variable is branched on only when no literal is
pure in the reduced formula (REF.py:186-208), so both of its literals occur in
an active clause and both occurrence lists are non-empty.  Empty lists are
covered for propagated literals (root units whose negation occurs nowhere)."""
import random

import pytest

import oracle
from satmi import _capi, cnf
from satmi.dpll import dpll_batch

pytestmark = pytest.mark.gpu

CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")
SPLITS = [_capi.SPLIT_OFF, _capi.SPLIT_ALWAYS]

_oracle_cache = {}


def _oracle(name, fs):
    """The oracle's results of a family, computed once and shared by its cases."""
    if name not in _oracle_cache:
        _oracle_cache[name] = [oracle.dpll(f, "sound", max_solutions=1, sol_cap=1) for f in fs]
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


def _check(name, fs, split):
    n = max(abs(l) for f in fs for c in f for l in c)
    m = max(len(f) for f in fs)
    L = max(sum(len(c) for c in f) for f in fs)
    assert all(1 <= len(c) <= 3 for f in fs for c in f)
    _capi.set_kernel(_capi.KERNEL_INC)
    try:
        kern, lds, _ = _capi.plan(n, m, L, 3)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    assert kern == _capi.KERNEL_INC and lds == 5108, "not dpll_fixed_kernel's shape class"
    want = _oracle(name, fs)
    r = _run(fs, _capi.KERNEL_INC, split)
    for b, o in enumerate(want):
        assert int(r.status[b]) == o["status"], (name, b)
        got = r.counter_dict(b)
        for k in CTR:
            assert got[k] == o["counters"][k], (name, b, k, fs[b] if len(fs[b]) <= 40 else None)
        model = o["solutions"][:1]
        assert r.solutions(b) == model, (name, b)
        if model:
            assert int(r.sol_len[b, 0]) == len(model[0]), (name, b)
    if split == _capi.SPLIT_OFF:   # rounds: one search per wave, the same count as the general kernel's
        rg = _run(fs, _capi.KERNEL_GENERAL, _capi.SPLIT_OFF)
        assert (r.counters[:, :7] == rg.counters[:, :7]).all(), name
    return want


# ---- malformed-but-legal clauses (repeats, tautologies, padding)

def _malformed(seed, count):
    rng = random.Random(seed)
    fs = [[[1], [1, 1], [-1, 1, 1]], [[1, 1, 1], [-1, -1]], [[-1, 1], [1, -1, 1]]]   # formulas of one variable
    while len(fs) < count:
        n = rng.randint(3, 12)
        skip = rng.randint(1, n - 1)   # this variable occurs nowhere (n itself occurs: the formula's size)
        vs = [v for v in range(1, n + 1) if v != skip]
        lit = lambda: rng.choice(vs) * rng.choice((1, -1))   # noqa: E731
        f = [[n * rng.choice((1, -1)), lit()]]
        for _ in range(rng.randint(4, 39)):
            kind = rng.random()
            if kind < 0.10:
                c = [lit()]
            elif kind < 0.30:
                c = [lit(), lit()]
            elif kind < 0.45:   # a literal twice, in any two slots
                a, b = lit(), lit()
                c = [a, a, b]
                rng.shuffle(c)
            elif kind < 0.60:   # x or not x or y, in any order
                a, b = lit(), lit()
                c = [a, -a, b]
                rng.shuffle(c)
            else:               # sampled with replacement: repeats and tautologies by chance
                c = [lit(), lit(), lit()]
            f.append(c)
        rng.shuffle(f)
        fs.append(f)
    return fs


@pytest.mark.parametrize("split", SPLITS)
def test_malformed_clauses_parity(split):
    fs = _malformed(4401, 64)
    assert len(fs) == 64 and all(len(f) <= 40 for f in fs)
    assert max(abs(l) for f in fs for c in f for l in c) <= 12
    cls = [c for f in fs for c in f]
    assert any(len(c) == 1 for c in cls) and any(len(c) == 2 for c in cls)
    assert any(len(c) == 3 and len(set(c)) == 2 and not any(-l in c for l in c) for c in cls)   # a literal twice
    assert any(len(c) == 3 and any(-l in c for l in c) for c in cls)                            # a tautology
    assert any(max(abs(l) for c in f for l in c) == 1 for f in fs)                               # one variable
    assert any(set(range(1, max(abs(l) for c in f for l in c) + 1)) - {abs(l) for c in f for l in c} for f in fs)
    want = _check("malformed", fs, split)
    assert sum(o["counters"]["decisions"] > 0 for o in want) >= 8
    assert sum(o["counters"]["conflicts"] > 0 for o in want) >= 8
    assert sum(o["counters"]["unit_props"] > 0 for o in want) >= 32


# ---- slot coverage: the propagated literal in slot 0, 1, 2 of the clause it makes unit / empty

def _perms(c):
    a, b, d = c
    return [[a, b, d], [a, d, b], [b, a, d], [b, d, a], [d, a, b], [d, b, a]]


def _slot_formulas():
    """Root chains over r=1, q=2, a=3, a2=4, b=5 (+ free 6..8): round 1 assigns
    the root units r (and q), round 2 assigns a (and a2) from [-r, a], and in
    round 3 the clause under test, reached through the list of -a, becomes
    unit (b is its free slot) or empty, -a sitting in each slot in turn."""
    r, q, a, a2, b = 1, 2, 3, 4, 5
    tail = [[6, 7, 8], [-6, -7, 8], [6, -7, -8], [-6, 7, -8], [b, 6, -8]]   # decisions after the chain
    fs, kinds = [], []
    for p in _perms([-a, b, -r]):          # unit: false slots -a (this batch) and -r (an older batch)
        fs.append([[r], [-r, a], p] + tail)
        kinds.append("unit")
    for p in ([-a, b], [b, -a]):           # unit: the third slot is padding
        fs.append([[r], [-r, a], p] + tail)
        kinds.append("unit")
    for p in ([-a, -a, b], [-a, b, -a], [b, -a, -a], [-a, b, b], [b, -a, b], [b, b, -a]):   # repeats of either literal
        fs.append([[r], [-r, a], p] + tail)
        kinds.append("unit" if p.count(b) == 1 else "open")   # b twice: two free slots, not unit
    for p in _perms([-a, -r, -q]):         # empty: emptied by a, the latest of its literals
        fs.append([[r], [q], [-r, a], p] + tail)
        kinds.append("empty")
    for p in _perms([-a, -a2, -r]):        # empty, two literals of one batch: the later one (a2) emptied it
        fs.append([[r], [-r, a], [-r, a2], [-a, 6, 7], p] + tail)
        kinds.append("empty2")
    for p in _perms([-a2, -a, b]):         # unit, reached from two batch literals (two lanes, one entry)
        fs.append([[r], [-r, a], [-r, a2], p] + tail)
        kinds.append("unit")
    for p in ([-a], [-a, -r], [-r, -a]):   # empty with padding
        fs.append([[r], [-r, a], p] + tail)
        kinds.append("empty")
    return fs, kinds


@pytest.mark.parametrize("split", SPLITS)
def test_slot_coverage_parity(split):
    fs, kinds = _slot_formulas()
    assert max(abs(l) for f in fs for c in f for l in c) == 8
    want = _check("slots", fs, split)
    for f, kind, o in zip(fs, kinds, want):
        c = o["counters"]
        if kind in ("empty", "empty2"):   # a root conflict: the search ends in the root's propagation
            assert o["status"] == _capi.DPLL_EXHAUSTED and c["conflicts"] == 1 and c["decisions"] == 0, f
            assert c["nodes"] == 1 and c["solutions"] == 0, f
        elif kind == "unit":  # b was propagated at the root, in round 3
            assert 5 in o["root_assign"] and 3 in o["root_assign"], f
            assert o["root_assign"].index(3) < o["root_assign"].index(5), f
    # the two-literal batch: the reference stops at the later literal (a2), so both count as propagations
    both = [o for kind, o in zip(kinds, want) if kind == "empty2"]
    assert len(both) == 6 and all(o["counters"]["unit_props"] == 3 for o in both)


# ---- decision path

def _tseitin(vertices, seed):
    """Parity constraints of a random 3-regular graph with odd total charge:
    UNSAT, every variable in both polarities (no pure literals), 4 clauses of
    3 literals per vertex -- a long search in a small formula."""
    rng = random.Random(seed)
    while True:
        stubs = [v for v in range(vertices) for _ in range(3)]
        rng.shuffle(stubs)
        edges = [(stubs[i], stubs[i + 1]) for i in range(0, len(stubs), 2)]
        if all(a != b for a, b in edges) and len({frozenset(e) for e in edges}) == len(edges):
            break
    inc = [[] for _ in range(vertices)]
    for i, (a, b) in enumerate(edges):
        inc[a].append(i + 1)
        inc[b].append(i + 1)
    f = []
    for v in range(vertices):
        charge = 1 if v == 0 else 0
        for s in range(8):
            bits = [(s >> j) & 1 for j in range(3)]
            if sum(bits) % 2 != charge:
                f.append([(-l if bt else l) for l, bt in zip(inc[v], bits)])
    return f


def _decision_formulas():
    rng = random.Random(77)
    no_units = []
    for _ in range(12):   # 3-literal clauses only: the first round of the search is a decision
        n = rng.randint(6, 12)
        no_units.append([[v * rng.choice((1, -1)) for v in rng.sample(range(1, n + 1), 3)]
                         for _ in range(rng.randint(4 * n, 5 * n))][:40])
    only_units = [[[1]], [[1], [-2], [-1, 3], [2, -3, 4]], [[3], [-3, 2], [-2, 1], [-1, -3, 4]],
                  [[1], [2], [3], [-1, -2, -3]]]   # the last: a root conflict
    # both branches of the first decision conflict at once: False follows True immediately
    flip = [[[1, 2], [1, -2], [-1, 2], [-1, -2]],
            [[1, 2, 3], [1, 2, -3], [1, -2, 3], [1, -2, -3], [-1, 2, 3], [-1, 2, -3], [-1, -2, 3], [-1, -2, -3]],
            [[1, 2], [1, -2], [-1, 3], [-1, -3], [2, 3, 1]]]
    return no_units, only_units, flip


@pytest.mark.parametrize("split", SPLITS)
def test_decision_entry_parity(split):
    no_units, only_units, flip = _decision_formulas()
    fs = no_units + only_units + flip
    want = _check("decisions", fs, split)
    a, b = len(no_units), len(no_units) + len(only_units)
    for o in want[:a]:
        assert o["root_assign"] == [] and (o["counters"]["decisions"] > 0 or o["counters"]["pure_assigns"] > 0)
    assert sum(o["counters"]["decisions"] > 0 for o in want[:a]) >= 8
    assert sum(o["counters"]["conflicts"] > 0 for o in want[:a]) >= 4
    for o in want[a:b]:
        assert o["counters"]["decisions"] == 0 and o["counters"]["unit_props"] > 0
    for o in want[b:]:
        assert o["status"] == _capi.DPLL_EXHAUSTED
        assert o["counters"]["decisions"] >= 2 and o["counters"]["conflicts"] >= 2


@pytest.mark.parametrize("split", SPLITS)
def test_decision_epoch_wraparound_parity(split):
    """One search of > 70,000 decisions (a parity formula of 42 variables and
    112 clauses): every decision takes a fresh 16-bit epoch through
    next_decision_epoch, so the stamps are reset at least once while decision
    literals are stamped by assign_decision."""
    fs = [_tseitin(28, 1)]
    want = _check("epoch", fs, split)
    assert want[0]["status"] == _capi.DPLL_EXHAUSTED
    assert want[0]["counters"]["decisions"] >= 70000, want[0]["counters"]


# ---- batch boundaries of the incremental unit scan

BATCH_SHAPES = [(1, 3), (2, 6), (16, 40), (17, 40), (2, 64), (2, 65), (16, 64), (17, 65), (1, 64), (1, 65)]


def _batch_formula(rng, B, T):
    """B root unit clauses [u_i] -- the first batch, B literals -- and clauses
    holding T negations -u_i in all (the occurrence entries the next unit scan
    walks: T touched clauses, one per entry), over 10 further variables."""
    us = list(range(1, B + 1))
    ys = list(range(B + 1, B + 11))
    y = lambda: rng.choice(ys) * rng.choice((1, -1))   # noqa: E731
    f = [[u] for u in us]
    t = 0
    while t < T:
        u = us[t % B]
        kind = rng.random()
        if kind < 0.25 and B > 1 and t + 2 <= T:   # reached from two batch literals
            c = [-u, -rng.choice([x for x in us if x != u]), y()]
            t += 2
        elif kind < 0.45:                          # unit in the next round
            c = [-u, y()]
            t += 1
        else:
            c = [-u, y(), y()]
            t += 1
        rng.shuffle(c)
        f.append(c)
    f += [[y(), y(), y()] for _ in range(12)]
    head, rest = f[:B], f[B:]
    rng.shuffle(rest)
    cut = rng.randint(0, len(rest))   # the unit clauses in order, the others around them
    return rest[:cut] + head + rest[cut:]


def _entries(f, batch):
    """Occurrence entries of the negations of `batch` (a clause counts once per literal code)."""
    return sum(1 for lit in batch for c in f if -lit in c)


@pytest.mark.parametrize("split", SPLITS)
def test_batch_boundaries_parity(split):
    rng = random.Random(9090)
    fs = []
    for B, T in BATCH_SHAPES:
        for _ in range(4):
            f = _batch_formula(rng, B, T)
            units = [c[0] for c in f if len(c) == 1]
            assert units == list(range(1, B + 1)) and _entries(f, units) == T, (B, T)
            fs.append(f)
    fs.append(cnf.uniform_ksat(1, 127, 448, 3, seed=127448).instance(0))   # the class limits
    assert len(fs[-1]) == 448 and max(abs(l) for c in fs[-1] for l in c) == 127
    want = _check("batches", fs, split)
    for (B, T), i in zip(BATCH_SHAPES, range(0, len(want), 4)):
        for o in want[i:i + 4]:   # the whole first batch was assigned (or a later round's conflict cut the search)
            assert o["counters"]["unit_props"] >= B or o["counters"]["conflicts"] > 0, (B, T)
        assert any(len(o["root_assign"]) > B for o in want[i:i + 4]), (B, T)   # units found by the scan under test
    assert want[-1]["counters"]["decisions"] > 0
