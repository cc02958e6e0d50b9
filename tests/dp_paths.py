"""Formulas that drive the Davis-Putnam kernels (csrc/dp.hip) out of the one
layout class the rest of the suite runs in (at most 30 variables: one key
word per sign, every table in LDS, lists of a few thousand clauses), shared by
tests/test_dp_paths.py (CPU: every row has the variable count, the key width
and the sizes it claims, and the oracle finishes it) and
tests/test_dp_paths_gpu.py (GPU: every row exact against the oracle).

What decides a path in csrc/dp.hip, in the kernels' terms:

  V     distinct variables (the dense index is the rank of the id); K = 2 *
        ceil(V / 64) key words per clause.  K = 2, 4, 6, 8 have their own
        instances of the subset-test kernels, K >= 10 the run-time-width one;
        the inline form holds at most 8 key words in registers;
  V <= 255    the model set of variables.pop() fits LDS, else global scratch;
  V <= 2048   the first-position table, the rank loop and the insertion order
        sit in LDS, else in global memory (and no step runs inline);
  ids   every id below the variable set's final table size: pop() is the
        smallest id (`mul = 1`); else the set is built in insertion order
        (`mul = 37`);
  ncl   > 16,384 clauses: the split re-reads its flags; >= 65,536: three
        scans, not the packed one (pos count | neg count << 16);
  sizes past a fresh workspace's capacities: the step is run again (resumes).
"""
import functools
import random

import oracle
from satmi import cnf


def key_words(V):
    return 2 * ((V + 63) // 64)


def variables(f):
    return {abs(l) for c in f for l in c}


def _signed(rng, vs):
    return [v if rng.random() < 0.5 else -v for v in vs]


def sparse3(n, m, seed, mul, first=1):
    """m random 3-literal clauses over exactly the n variables first ..
    first + n - 1 (a shuffled cover of them, the rest uniform), ids times mul."""
    rng = random.Random(seed)
    ids = list(range(first, first + n))
    perm = ids[:]
    rng.shuffle(perm)
    f = []
    for i in range(0, n, 3):
        vs = perm[i:i + 3]
        while len(vs) < 3:
            v = rng.choice(ids)
            if v not in vs:
                vs.append(v)
        f.append(_signed(rng, vs))
    assert m >= len(f)
    while len(f) < m:
        f.append(_signed(rng, rng.sample(ids, 3)))
    rng.shuffle(f)
    assert variables(f) == set(ids)
    return [[l * mul for l in c] for c in f]


def chain(n, perm_seed, sat):
    """[x1], [-x1, x2], .., [-x(n-1), xn] (+ [-xn] unless sat): every list of
    the elimination is of linear size, the verdict is reached.  Variables
    renamed by a seeded permutation and times 37, clause order shuffled."""
    rng = random.Random(perm_seed)
    img = list(range(1, n + 1))
    rng.shuffle(img)
    x = [0] + [37 * v for v in img]
    f = [[x[1]]] + [[-x[i], x[i + 1]] for i in range(1, n)]
    if not sat:
        f.append([-x[n]])
    rng.shuffle(f)
    assert len(variables(f)) == n
    return f


def disjoint(copies, seed, mul=37):
    """The union of `copies` random formulas (n = 10, m = 30, 3 literals) on
    disjoint variable ranges, interleaved clause by clause: V = 10 * copies,
    and every step stays inside one small formula."""
    rng = random.Random(seed)
    parts = []
    for i in range(copies):
        while True:
            ids = list(range(10 * i + 1, 10 * i + 11))
            p = [_signed(rng, rng.sample(ids, 3)) for _ in range(30)]
            if variables(p) == set(ids):
                break
        parts.append(p)
    f = [parts[i][j] for j in range(30) for i in range(copies)]
    assert len(variables(f)) == 10 * copies
    return [[l * mul for l in c] for c in f]


def long_clauses(n, seed):
    """sparse3(n, 1.4 n) plus six clauses of 20-40 literals over consecutive
    dense indices that straddle a key-word boundary (63/64, and 127/128 where n
    reaches it), one tautological clause whose v / -v sits at dense index 64,
    and one duplicate clause; ids times 37."""
    rng = random.Random(seed)
    f = sparse3(n, int(1.4 * n), seed, 1)
    bounds = [b for b in (64, 128) if b + 4 < n]
    for k in range(6):
        L = rng.randint(20, 40)
        b = bounds[k % len(bounds)]
        start = max(0, min(b - rng.randint(5, L - 5), n - L))
        assert start <= b - 1 and start + L - 1 >= b
        f.insert(rng.randrange(len(f)), _signed(rng, range(start + 1, start + L + 1)))   # id = dense index + 1
    f.insert(rng.randrange(len(f)), [65, -65, rng.randint(1, 60)])
    f.append(list(f[3]))
    assert len(variables(f)) == n
    return [[l * 37 for l in c] for c in f]


def wide_pairs():
    """66,000 clauses, ids 1 .. 6,002 (below the variable set's table size:
    variable 1 is popped first).  Variable 1 occurs positively in 300 clauses
    and negatively in 300: 90,000 pairs in the first step, more than a fresh
    workspace's 65,536.  297 of the positive clauses hold 2 and every negative
    one -2, so all but 3 x 300 resolvents are tautologies (the oracle's
    unique_new is quadratic in the others); the 900 kept are 4-literal clauses
    holding -2, so the second step has an empty pos list."""
    rng = random.Random(66)
    f = sparse3(6000, 65400, 660, 1, first=3)
    pos = [[1, 2, rng.randint(3, 6002)] for _ in range(297)] + \
          [[1] + rng.sample(range(3, 6003), 2) for _ in range(3)]
    neg = [[-1, -2, -rng.randint(3, 6002)] for _ in range(300)]
    rng.shuffle(pos)
    for k, c in enumerate(pos + neg):
        f.insert((k * 109) % len(f), c)
    assert len(f) == 66000 and max(variables(f)) == 6002
    return f


def packed_sign():
    """40,000 clauses (fewer than 65,536: the packed scan, runs of 40 clauses
    per thread) of which 33,050 hold -1: a neg count of 2^15 or more sets the
    sign bit of the packed word.  One positive clause [1, 2, x]; 33,000
    negative ones hold -2 (tautologies), 50 do not."""
    rng = random.Random(40)
    f = sparse3(3000, 6949, 400, 1, first=3)
    neg = [[-1, -2] + rng.sample(range(3, 3003), 2) for _ in range(33000)] + \
          [[-1] + rng.sample(range(3, 3003), 2) for _ in range(50)]
    rng.shuffle(neg)
    f = f + neg
    rng.shuffle(f)
    f.insert(len(f) // 2, [1, 2, 77])
    assert len(f) == 40000
    return f


def long_pairs():
    """Variable 1 (the smallest id, popped first) in 24 positive and 24
    negative clauses of 21 literals, all other literals positive: 576 kept
    resolvents of about 40 literals, 1,024 arena ints each (capR = 512) --
    more than a fresh arena -- and tables too large for the assembly's LDS
    scratch; beside sparse3 on 70 other variables, none of whose clauses can
    be a subset of a resolvent (V = 141, K = 6)."""
    rng = random.Random(24)
    f = sparse3(70, 98, 240, 1, first=2)
    for s in (1, -1):
        for _ in range(24):
            f.insert(rng.randrange(len(f)), [s] + rng.sample(range(72, 142), 20))
    return f


def inline_scratch():
    """Variable 1 in 10 positive and 10 negative clauses of 33 literals: 100
    kept resolvents whose tables (capA = capB = 512, capR = 1024) are built in
    the assembly's global scratch, 2,048 ints each -- more than a fresh
    workspace's -- while the arena (200 clauses of up to 33 literals) and the
    clause list have room: with K = 8 the inline form would run the step, and
    must not hand it to the assembly before the scratch has grown."""
    rng = random.Random(33)
    f = sparse3(100, 180, 330, 1, first=2)
    for s in (1, -1):
        for _ in range(10):
            f.insert(rng.randrange(len(f)), [s] + rng.sample(range(102, 202), 32))
    return f


def many_resolvents():
    """20 variables, many resolvents per step (as test_dp_gpu's thread test):
    stale table slots or stamps of a wider solve before it would show."""
    return cnf.uniform_ksat(1, 12, 50, 3, seed=3).instance(0) + [[13 + i, -(14 + i)] for i in range(7)] + [[20, 13]]


# name -> (builder, step_limit (0: to the verdict), V)
ROWS = {}


def _row(name, build, step_limit, V):
    ROWS[name] = (build, step_limit, V)


# 1. key widths: each boundary of V and its neighbour, K = 2, 4, 6, 8, 10
for _V in (64, 65, 128, 129, 192, 193, 256, 257):
    for _mul in (37, 1):
        _row(f"sparse3_{_V}_x{_mul}", lambda V=_V, mul=_mul: sparse3(V, int(1.4 * V), V, mul), 10, _V)
    for _sat in (True, False):
        _row(f"chain_{_V}_{'sat' if _sat else 'unsat'}", lambda V=_V, sat=_sat: chain(V, V, sat), 0, _V)
for _V in (70, 130, 200, 260):
    _row(f"disjoint_{_V}", lambda V=_V: disjoint(V // 10, V), 0, _V)
for _V in (70, 200):
    _row(f"long_{_V}", lambda V=_V: long_clauses(V, V), 10, _V)
KEY_WIDTH_ROWS = tuple(ROWS)

# 2. the model set of variables.pop(): 255 the last size in LDS, 256 the first in global scratch
for _V in (255, 256):
    _row(f"popset_{_V}", lambda V=_V: sparse3(V, int(1.4 * V), 1000 + V, 37), 10, _V)
_row("chain_300_sat", lambda: chain(300, 300, True), 0, 300)
_row("chain_300_unsat", lambda: chain(300, 301, False), 0, 300)
POPSET_ROWS = ("popset_255", "popset_256", "chain_300_sat", "chain_300_unsat")

# 3. the first-position table: 2,048 the last size in LDS.  chain(2049) to its
# verdict is 2,049 steps, each a serial build of the model set in global
# memory: capped at 64 steps on both sides
for _V in (2048, 2049):
    for _mul in (37, 1):
        _row(f"firstpos_{_V}_x{_mul}", lambda V=_V, mul=_mul: sparse3(V, int(1.4 * V), V, mul), 8, _V)
_row("chain_2049_unsat", lambda: chain(2049, 2049, False), 64, 2049)
FIRSTPOS_ROWS = tuple(n for n in ROWS if n.startswith("firstpos_")) + ("chain_2049_unsat",)

# 4. large clause lists
_row("list_20000", lambda: sparse3(2500, 20000, 25, 1), 3, 2500)
_row("list_70000", lambda: sparse3(6000, 70000, 60, 1), 3, 6000)
_row("wide_pairs", wide_pairs, 3, 6002)
_row("packed_sign", packed_sign, 3, 3002)
LARGE_ROWS = ("list_20000", "list_70000", "wide_pairs", "packed_sign")

# 5. key-width changes on one workspace: V = 20, 70, 300, 20, 130, 20
_row("many_20", many_resolvents, 0, 20)
WIDTH_CHANGE_SEQUENCE = ("many_20", "disjoint_70", "chain_300_unsat", "many_20", "disjoint_130", "many_20")

# 6. resumes
_row("php65", lambda: cnf.pigeonhole(5), 0, 30)
_row("long_arena", long_pairs, 3, 141)
_row("inline_scratch", inline_scratch, 3, 201)


@functools.lru_cache(maxsize=None)
def row_formula(name):
    return ROWS[name][0]()


@functools.lru_cache(maxsize=None)
def row_oracle(name):
    """The oracle's recorded run of a row, once per process."""
    return oracle.dp(row_formula(name), step_limit=ROWS[name][1], record=True, rec_cap=1 << 22)


# ---- a step's sizes, from the oracle's record, and what a fresh workspace holds

def cap_for(u):
    """csrc/dp.hip cap_for: table slots given to a set of u keys."""
    c = 8
    while c <= 8 * u:
        c <<= 1
    return c


def step_sizes(name):
    """Per recorded step of the row: (np, nn, nr, nkept, mxA, mxB) -- the pos /
    neg / rem lists, the kept resolvents, the longest pos and neg clause."""
    f, o = row_formula(name), row_oracle(name)
    cur = [set(c) for c in f]
    out = []
    for var, nxt in zip(o["vars"], o["clauses"]):
        pos = [c for c in cur if var in c]
        neg = [c for c in cur if -var in c]
        nr = sum(1 for c in cur if var not in c and -var not in c)
        out.append((len(pos), len(neg), nr, len(nxt) - nr, max(map(len, pos), default=0), max(map(len, neg), default=0)))
        cur = [set(c) for c in nxt]
    return out


RESUME_KEYS = ("pairs", "clauses", "arena", "scratch")


def forced_resumes(name):
    """The buffers that a solve of the row on a FRESH workspace must outgrow
    (a capacity only moves when its own resume runs, so a step that needs more
    than the fresh capacity proves one).  The fresh capacities are
    satmi_dp_host's first requests, each half as much again (DevBuf::grow):
    65,536 pairs (the table has two slots per pair); 1.5 * max(1.5 n, 1024)
    clauses; 1.5 * max(4 * arena0, 65536) arena ints, arena0 = n * 2 *
    cap_for(longest clause); 1.5 * 65,536 ints of assembly scratch."""
    f = row_formula(name)
    n = len(f)
    ncl_cap = 3 * max(n + n // 2, 1024) // 2
    arena0 = n * 2 * cap_for(max(len(c) for c in f))
    arena_cap = 3 * max(4 * arena0, 65536) // 2
    top = arena0
    forced = set()
    for np_, nn, nr, nkept, mxA, mxB in step_sizes(name):
        if np_ * nn > 65536:
            forced.add("pairs")
        if nr + nkept > ncl_cap:
            forced.add("clauses")
        top += nkept * 2 * cap_for(mxA + mxB)
        if top > arena_cap:
            forced.add("arena")
        if nkept * 2 * (cap_for(mxA) + cap_for(mxB)) > 98304:
            forced.add("scratch")
    return forced


# row -> the resume it is there for
RESUME_ROWS = {"wide_pairs": ("pairs", "scratch"), "php65": ("pairs", "clauses", "arena", "scratch"),
               "long_arena": ("arena", "scratch"), "inline_scratch": ("scratch",)}


def py_size_after(n):
    """Table slots of a CPython set after n distinct insertions into an empty one."""
    mask = 7
    while True:
        thr = (mask * 3 + 4) // 5
        if n < thr:
            return mask + 1
        minused = thr * 2 if thr > 50000 else thr * 4
        ns = 8
        while ns <= minused:
            ns <<= 1
        mask = ns - 1
