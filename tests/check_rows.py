"""The model check's rule in plain Python, and the hand-built rows of its tests
(tests/test_check.py holds the evaluator to brute force; tests/test_check_gpu.py
holds the kernel to the evaluator).

A literal l is TRUE if l is in the row, FALSE if -l is in the row and l is not,
else UNASSIGNED.  A clause is satisfied if some literal is true, falsified if
every literal is false (the empty clause always is), else undetermined.  A
literal of the row that is 0, INT32_MIN or beyond max_vars is ignored and
flagged."""
import random

I32_MIN = -(2 ** 31)
CONTRADICTORY, BAD_LITERAL = 1, 2
SHORT_MAX = 8   # csrc/check.hip's CK_SHORT_MAX: the longest clause of the lane-per-clause form
MAX_VARS = 524287   # SATMI_CHECK_MAX_VARS


def max_vars_of(formula, rows=()):
    """What satmi_check_models_host computes: the largest variable of the formula and the rows."""
    return max([abs(l) for c in formula for l in c] + [abs(l) for r in rows for l in r if l != I32_MIN] + [0])


def evaluate(formula, row, max_vars=None):
    """[falsified, undetermined, first_falsified, flags] of `row` against `formula`."""
    if max_vars is None:
        max_vars = max_vars_of(formula, [row])
    flags = 0
    held = set()
    for l in row:
        if l == 0 or l == I32_MIN or abs(l) > max_vars:
            flags |= BAD_LITERAL
        else:
            held.add(l)
    if any(-l in held for l in held):
        flags |= CONTRADICTORY
    falsified = undetermined = 0
    first = -1
    for i, c in enumerate(formula):
        if any(l in held for l in c):
            continue
        if all(-l in held and l not in held for l in c):
            falsified += 1
            if first < 0:
                first = i
        else:
            undetermined += 1
    return [falsified, undetermined, first, flags]


def is_ok(words):
    return words[0] == 0 and words[1] == 0 and words[3] == 0


def expected(formulas, rows_of, cap, max_vars=None):
    """The [B][cap][4] words of a batch: rows_of[b] = the rows checked of formula b,
    the slots past them zeros; max_vars=None: per call, over the whole batch (the host form's)."""
    if max_vars is None:
        max_vars = max([max_vars_of(f, r) for f, r in zip(formulas, rows_of)] + [0])
    return [[evaluate(f, r, max_vars) for r in rows] + [[0, 0, 0, 0]] * (cap - len(rows))
            for f, rows in zip(formulas, rows_of)]


# ---- test 1: edge rows, (formula, row) pairs of one batch
EDGE_CASES = [
    ([], [1, -2]),                               # empty formula: nothing to falsify
    ([], []),                                    # ... and an empty row
    ([[1, 2], [], [-1]], [1, 2]),                # an empty clause is falsified under any row (and [-1] here)
    ([[1, 2], [-1, 3]], []),                     # empty row: every clause undetermined
    ([[1], [-2], [3]], [1, -2, -3]),             # unit clauses: two satisfied, one falsified
    ([[1], [-2], [3]], [1, -2]),                 # ... one undetermined
    ([[1, -1], [2]], [2]),                       # tautological clause, its variable unassigned: undetermined
    ([[1, -1], [2]], [-1, 2]),                   # ... satisfied through -1
    ([[1, 1, 2], [-1, -1]], [-1, -2]),           # repeated literal in a clause
    ([[1, 2], [-1]], [1, 1, 1, 2]),              # repeated literal in the row
    ([[1], [-1], [2], [-2, 3]], [1, -1, -2]),    # contradictory row: +1 and -1 both true, flags 1
    ([[1, 2], [-2]], [-1, 0, 2]),                # literal 0 in the row: ignored, flags 2
    ([[1, 2], [-2]], [I32_MIN, -2, 1]),          # INT32_MIN in the row
    ([[1, 2], [3]], [1, 9, -3]),                 # beyond max_vars (3 when the caller says so): flags 2
    ([[1, 2], [3]], [-9, 9, 3, -3]),             # bad and contradictory: flags 3
]
EDGE_MAX_VARS = 3   # the device form's max_vars for the edge batch: the formulas' own


def random_mix(seed=5, count=300):
    """The 300-formula mix of test_dpll_gpu.py::test_sound_mode_matches_oracle_small
    (n 3-14, clauses of 1-5 literals), drawn the same way."""
    rng = random.Random(seed)
    fs = []
    for i in range(count):
        n = rng.randint(3, 14)
        m = rng.randint(1, 70)
        k = rng.randint(1, 5)
        fs.append([[v if rng.random() < 0.5 else -v
                    for v in rng.sample(range(1, n + 1), min(k, n) if i % 3 else rng.randint(1, min(k, n)))]
                   for _ in range(m)])
    return fs


# ---- test 4: clause lengths on both sides of the two forms' threshold
CLAUSE_LENGTHS = (1, SHORT_MAX, SHORT_MAX + 1, 63, 64, 65, 300)


def length_case(k):
    """Three clauses of k literals over variables 1 .. 3k and the row that leaves them
    satisfied only by the last literal, falsified, and undetermined only through the last."""
    a, b, c = (list(range(1 + j * k, 1 + (j + 1) * k)) for j in range(3))
    formula = [a, b, c]
    row = [-v for v in a[:-1]] + [a[-1]] + [-v for v in b] + [-v for v in c[:-1]]
    return formula, row   # -> [1, 1, 1, 0]


# ---- test 5: clause counts around the 64-clause step
CLAUSE_COUNTS = (0, 1, 63, 64, 65, 128, 129)


def count_cases():
    """(formula, row, want) with m two-literal clauses over variables 1, 2 satisfied by the
    row [1, -2] but for one falsified clause at each of the indices 0, 63, 64, m - 1 that
    exist, and for two falsified clauses (the smaller index wins)."""
    out = []
    row = [1, -2]
    for m in CLAUSE_COUNTS:
        spots = sorted({i for i in (0, 63, 64, m - 1) if 0 <= i < m})
        for falsified in [()] + [(i,) for i in spots] + ([(spots[1], spots[-1])] if len(spots) > 2 else []):
            f = [[-1, 2] if i in falsified else [1, 2] for i in range(m)]
            out.append((f, row, [len(falsified), 0, min(falsified, default=-1), 0]))
    return out


# ---- test 6: table reuse.  A clause is falsified only if the row holds the negation of
# every one of its literals, so over pairwise DISJOINT variable sets a bit that survived row k
# cannot satisfy a clause row k + 1 falsifies; what it can do is falsify a second clause ahead
# of the row's own, and satisfy a clause that is undetermined (reuse_disjoint pins both).  A
# stale bit satisfies the next row's falsified clause where consecutive rows hold the SAME
# variable with opposite signs (reuse_alternating).
def reuse_disjoint(nrows=8):
    """Row k = [-a_k, -b_k] over its own variables a_k = 2k + 1, b_k = 2k + 2; the formula has
    the clauses [a_k], [-b_k] for every k.  Row k alone: clause 2k falsified, 2k + 1
    satisfied, the other 2(nrows - 1) undetermined.  A bit left by row k - 1 would falsify
    clause 2k - 2 (a smaller first index, a count of 2) and satisfy clause 2k - 1."""
    formula, rows = [], []
    for k in range(nrows):
        formula += [[2 * k + 1], [-(2 * k + 2)]]
        rows.append([-(2 * k + 1), -(2 * k + 2)])
    return formula, rows   # row k -> [1, 2 * (nrows - 1), 2 * k, 0]


def reuse_alternating(nrows=8):
    """Rows [1, -2, -3], [-1, -2, -3], [1, ...] in turn against [[1], [-1], [2, 3]]: every row
    falsifies [2, 3] and one of the units, which the previous row's bit for variable 1
    would satisfy (and the row would read as contradictory)."""
    formula = [[1], [-1], [2, 3]]
    rows = [[1 if k % 2 == 0 else -1, -2, -3] for k in range(nrows)]
    return formula, rows   # row k -> [2, 0, 1 - k % 2, 0]
