"""The witness kernel's rule in plain Python, the reference's two solvers restated
with recording, and the hand-built cases of the tests (tests/test_witness.py holds
the evaluator to brute force; tests/test_witness_gpu.py holds the kernel to the
evaluator, words and rows).

An instance is a formula F of m clauses, a record R of P clauses and an ordered
list of stages (x, lo, hi), lo <= hi <= m + P: clause index c < m is formula
clause c, index m + j record clause j.  The assignment is total and every
variable starts False.  Stage (x, lo, hi), over the clauses of its range: a
clause with +x and -x is passed; with highest_only so is one whose largest
|literal| is not x; needP holds if some clause holds +x and every other literal
of it is false, needN likewise with -x; with both the stage is stuck; in every
case x becomes needP.  A literal 0, INT32_MIN or beyond max_vars is false (and a
magnitude) and sets BAD_LITERAL when it is in F or in a clause that a stage
reads; a stage whose variable is outside 1 .. max_vars is skipped and sets
BAD_STAGE.  After the last stage every clause of F is evaluated: MODEL iff none
is falsified.  The row holds one signed literal per distinct variable that occurs
in F with a good literal, ascending, the sign by the final value; beyond `stride`
it is cut and ROW_TRUNCATED set."""
import itertools
import random

I32_MIN = -(2 ** 31)
NOT_MODEL, MODEL = 0, 1
BAD_LITERAL, BAD_STAGE, ROW_TRUNCATED = 1, 2, 4
NWORDS = 6
SHORT_MAX = 8          # csrc/witness.hip's WT_SHORT_MAX: the longest clause of the lane-per-clause form
MAX_VARS = 524287      # SATMI_WITNESS_MAX_VARS


def max_vars_of(formula, record=()):
    """What satmi_witness_models_host computes: the largest variable of formula and record."""
    return max([abs(l) for c in formula for l in c] + [abs(l) for c in record for l in c] + [0])


def _is_bad(l, max_vars):
    return l == 0 or l == I32_MIN or abs(l) > max_vars


def evaluate(formula, record, stages, highest_only=False, max_vars=None, stride=None):
    """([status, stuck, first_stuck, flags, falsified, first_falsified], row_len, row) of one
    instance; the row is cut at `stride` (None: never)."""
    if max_vars is None:
        max_vars = max_vars_of(formula, record)
    m = len(formula)
    clauses = list(formula) + list(record)
    true = set()          # the variables that are True
    flags = 0
    if any(_is_bad(l, max_vars) for c in formula for l in c):
        flags |= BAD_LITERAL

    def holds(l):
        return not _is_bad(l, max_vars) and ((abs(l) in true) == (l > 0))

    stuck, first_stuck = 0, -1
    for t, (x, lo, hi) in enumerate(stages):
        if not 1 <= x <= max_vars:
            flags |= BAD_STAGE
            continue
        lo = min(max(lo, 0), len(clauses))                # (the device form clamps; the host form refuses)
        hi = min(max(hi, lo), len(clauses))
        need_p = need_n = False
        for c in clauses[lo:hi]:
            if any(_is_bad(l, max_vars) for l in c):
                flags |= BAD_LITERAL
            if x in c and -x in c:
                continue
            if highest_only and max([abs(l) for l in c] + [0]) != x:
                continue
            if any(holds(l) for l in c if l != x and l != -x):
                continue
            need_p |= x in c
            need_n |= -x in c
        if need_p and need_n:
            if stuck == 0:
                first_stuck = t
            stuck += 1
        (true.add if need_p else true.discard)(x)
    falsified = [i for i, c in enumerate(formula) if not any(holds(l) for l in c)]
    row = [v if v in true else -v
           for v in sorted({abs(l) for c in formula for l in c if not _is_bad(l, max_vars)})]
    n = len(row)
    if stride is not None and n > stride:
        flags |= ROW_TRUNCATED
        row = row[:stride]
    status = NOT_MODEL if falsified else MODEL
    return [status, stuck, first_stuck, flags, len(falsified), falsified[0] if falsified else -1], n, row


def expected(formulas, records, stages, highest_only=False, max_vars=None, stride=None):
    """([B][6] words, [B] row lengths, [B] rows); max_vars=None: per call, over the whole
    batch (the host form's)."""
    if max_vars is None:
        max_vars = max([max_vars_of(f, r) for f, r in zip(formulas, records)] + [0])
    got = [evaluate(f, r, s, highest_only, max_vars, stride) for f, r, s in zip(formulas, records, stages)]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


# ---- REF.py:63-130 restated with recording (the popped variable is any: the rule does not care)
def ref_resolution(formula):
    """(answer, the clauses every pass added, in order) of REF.py:63-95.  A clause set is a
    pair of bit masks (its positive variables, its negative ones): `(ci | cj) - {lit, -lit}`
    is the union without lit's variable whichever sign lit has, so a pair of clauses has one
    resolvent per variable on which they clash."""
    def masks(c):
        return (sum(1 << v for v in {l for l in c if l > 0}), sum(1 << -v for v in {l for l in c if l < 0}))

    def clause(p, n):
        return [l for v in range(1, max(p, n).bit_length()) for l in (v, -v) if (p if l > 0 else n) >> v & 1]

    clauses = [masks(c) for c in formula]
    seen = set(clauses)
    record = []
    while True:
        new = {}
        n = len(clauses)
        for i in range(n):
            pi, ni = clauses[i]
            for j in range(i + 1, n):
                pj, nj = clauses[j]
                clash = (pi & nj) | (ni & pj)
                while clash:
                    b = clash & -clash
                    clash ^= b
                    rp, rn = (pi | pj) & ~b, (ni | nj) & ~b
                    if rp & rn:
                        continue          # a tautology
                    if not rp | rn:
                        return False, record
                    if (rp, rn) not in seen:
                        new[rp, rn] = None
        if not new:
            return True, record
        seen.update(new)
        clauses.extend(new)
        record.extend(clause(p, n) for p, n in new)


def ref_davis_putnam(formula, rng=None):
    """(answer, the popped variables, the clause list after every completed step) of
    REF.py:98-130; the popped variable is the set's own pop, or `rng`'s choice."""
    clauses = [set(c) for c in formula]
    variables = {abs(l) for c in clauses for l in c}
    popped, lists = [], []
    while variables:
        var = rng.choice(sorted(variables)) if rng else variables.pop()
        popped.append(var)
        pos = [c for c in clauses if var in c]
        neg = [c for c in clauses if -var in c]
        rest = [c for c in clauses if var not in c and -var not in c]
        new = []
        for pc in pos:
            for nc in neg:
                res = (pc - {var}) | (nc - {-var})
                if any(-l in res for l in res):
                    continue
                if not res:
                    return False, popped, lists
                new.append(res)
        unique = []
        for nc in new:
            if not any(nc.issuperset(e) for e in rest + unique):
                unique.append(nc)
        clauses = rest + unique
        lists.append([sorted(c, key=lambda l: (abs(l), l < 0)) for c in clauses])
        variables = {abs(l) for c in clauses for l in c}
    return True, popped, lists


def elimination_stages(m, popped, lists):
    """satmi.witness.stages_of_elimination on the restatement's record."""
    lo, spans = m, [(0, m)]
    for group in lists:
        spans.append((lo, lo + len(group)))
        lo += len(group)
    return [(popped[k], *spans[k]) for k in range(len(lists) - 1, -1, -1)]


def resolution_stages(formula, record):
    """satmi.witness.stages_of_resolution on the restatement's record (highest_only)."""
    top = len(formula) + len(record)
    return [(v, 0, top) for v in sorted({abs(l) for c in list(formula) + list(record) for l in c})]


# ---- brute force (test_witness.py)
def satisfies(formula, row):
    """Whether the signed literals `row` (total over the formula's variables) satisfy it."""
    true = set(row)
    return all(any(l in true for l in c) for c in formula)


def satisfiable(formula):
    vs = sorted({abs(l) for c in formula for l in c})
    return any(satisfies(formula, [v if b else -v for v, b in zip(vs, bits)])
               for bits in itertools.product((False, True), repeat=len(vs)))


def random_formulas(seed, count, clean, nmax=6, mmax=14):
    """`count` formulas of <= nmax variables, <= mmax clauses of 1 .. 3 literals; clean: distinct
    variables in a clause; else repeated literals and +v, -v in one clause happen."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(1, nmax)
        f = []
        for _ in range(rng.randint(0, mmax)):
            k = rng.randint(1, 3)
            if clean:
                f.append([v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), min(k, n))])
            else:
                f.append([rng.choice((1, -1)) * rng.randint(1, n) for _ in range(k)])
        out.append(f)
    return out


# ---- the hand-built cases: (formula, record, stages, highest_only, want words, want row)
STUCK = ([[1], [-1]], [], [(1, 0, 2)], False, [NOT_MODEL, 1, 0, 0, 1, 1], [1])
EDGE_CASES = [
    STUCK,
    ([[1, 2]], [], [(1, 0, 1), (2, 0, 1)], True, [MODEL, 0, -1, 0, 0, -1], [-1, 2]),      # 1 is not the highest
    ([[1, 2]], [], [(1, 0, 1), (2, 0, 1)], False, [MODEL, 0, -1, 0, 0, -1], [1, -2]),     # ... and forced without the flag
    ([[1, -1, 2], [-2]], [], [(1, 0, 2)], False, [MODEL, 0, -1, 0, 0, -1], [-1, -2]),     # a tautologous clause forces nothing
    ([[1], [-1, 2]], [[-1]], [(1, 0, 1), (2, 0, 2), (1, 2, 3), (1, 0, 1)], False,
     [MODEL, 0, -1, 0, 0, -1], [1, 2]),                                                   # 1: True, then False, then True
    ([[1, 2], [-1, 3]], [[2, 3]], [(2, 0, 3)], False, [MODEL, 0, -1, 0, 0, -1], [-1, 2, -3]),   # 1, 3 vanish unstaged
    ([[1, 2], [3]], [[-3], [4]], [(3, 1, 3)], False, [NOT_MODEL, 1, 0, 0, 1, 0], [-1, -2, 3]),  # a range straddling m
    ([[1]], [], [(1, 1, 1), (1, 0, 0)], False, [NOT_MODEL, 0, -1, 0, 1, 0], [-1]),        # empty ranges
    ([[1], [2, -1]], [], [(1, 0, 1), (1, 0, 1), (2, 0, 2), (2, 0, 2)], False,
     [MODEL, 0, -1, 0, 0, -1], [1, 2]),                                                   # repeated ranges
    ([[1], []], [], [(1, 0, 2)], False, [NOT_MODEL, 0, -1, 0, 1, 1], [1]),                # the reference's unsound True
    ([], [], [], False, [MODEL, 0, -1, 0, 0, -1], []),                                    # no clause, no stage
    ([[2, 2, 1], [-2, -2]], [], [(1, 0, 2), (2, 0, 2)], False, [MODEL, 0, -1, 0, 0, -1], [1, -2]),   # repeated literals
]


def stage_size_case(n, at):
    """One stage of n clauses over variable 1 with the only forcing clause at index `at`: the
    others hold +1 beside a literal that is true (variable 2 is False, they hold -2)."""
    f = [[1, -2]] * n
    f[at] = [1, 2]
    return f, [], [(1, 0, n)], False


STAGE_SIZES = [(n, at) for n in (63, 64, 65, 129) for at in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)})]
CLAUSE_LENGTHS = (1, 8, 9, 64, 65, 130)


def length_case(k, base=0):
    """A clause of k literals, +x first and the decisive literal last: the k - 2 literals in
    between are false, the last one false in the first clause (x is forced) and true in the
    second (y is not).  Variables base + 1 .. base + k + 1; the stages decide the last literal's
    variable first."""
    x, y, last = base + 1, base + 2, base + k + 1
    mid = list(range(base + 3, base + k + 1))           # k - 2 variables, all False
    if k == 1:
        return [[x]], [], [(x, 0, 1)], False
    f = [[x] + mid + [-last], [y] + mid + [last], [last]]
    return f, [], [(last, 2, 3), (x, 0, 2), (y, 0, 2)], False


VARIABLE_IDS = (15, 16, 17, 31, 32, 33)


def variable_case(v):
    """Variables v - 1, v, v + 1 around a word or half-word boundary of the table: v is forced
    True through its neighbours' values, which differ."""
    f = [[v - 1], [-(v - 1), v, v + 1], [-(v + 1), -v, -(v - 1)]] if v > 1 else [[v]]
    return f, [], [(v - 1, 0, 1), (v, 0, 3), (v + 1, 0, 3)], False


def forty():
    """Forty instances over variables 1 .. 40 ordered so that a bit left in the table by one
    shows in the next one's row: instance i forces its variables True, instance i + 1 holds
    the same variables unstaged (False unless a bit survived), and so on in turn."""
    fs, rs, ss = [], [], []
    for i in range(40):
        vs = [1 + (i // 2 + k * 7) % 40 for k in range(3)]
        if i % 2 == 0:
            fs.append([[v] for v in vs] + [[vs[0], -vs[1]]])
            rs.append([[vs[2]]])
            ss.append([(v, 0, 5) for v in vs])
        else:
            fs.append([[-v, vs[0]] for v in vs[1:]] + [[-vs[0]]])
            rs.append([])
            ss.append([(vs[0], 0, 3)] if i % 4 == 1 else [])
    return fs, rs, ss
