"""The refutation check's rule in plain Python, and the hand-built cases of its
tests (tests/test_refute.py holds the evaluator to brute force;
tests/test_refute_gpu.py holds the kernel to the evaluator).

Lemma i of a proof is VERIFIED if assigning every literal of it false and
running unit propagation to a fixpoint over the formula and the lemmas before
it reaches a conflict: a clause whose literals are all false, or a variable
needed with both signs.  An earlier lemma is a premise whether or not it
verified.  A lemma with +v and -v is verified trivially (flag TAUTOLOGY).
Checking ends with the first empty lemma.  A literal 0, INT32_MIN or beyond
max_vars is bad: a premise that holds one is skipped, a lemma that holds one
fails, and a bad literal in the formula or in a checked lemma sets BAD_LITERAL."""
import random

I32_MIN = -(2 ** 31)
FAILED, PROVEN, OPEN = 0, 1, 2
TAUTOLOGY, BAD_LITERAL = 1, 2
SHORT_MAX = 8        # csrc/refute.hip's RF_SHORT_MAX: the longest clause of the lane-per-clause form
MAX_VARS = 32767     # SATMI_REFUTE_MAX_VARS


def max_vars_of(formula, proof=()):
    """What satmi_check_refutations_host computes: the largest variable of formula and proof."""
    return max([abs(l) for c in formula for l in c] + [abs(l) for c in proof for l in c] + [0])


def _is_bad(l, max_vars):
    return l == 0 or l == I32_MIN or abs(l) > max_vars


def propagates_to_conflict(premises, assumed):
    """Whether unit propagation over the clause sets `premises` from the true literals
    `assumed` reaches a conflict.  A naive fixpoint loop: one clause at a time."""
    true = set(assumed)
    if any(-l in true for l in true):
        return True
    changed = True
    while changed:
        changed = False
        for c in premises:
            if any(l in true for l in c):
                continue
            free = {l for l in c if -l not in true}
            if not free:
                return True
            if len(free) == 1:
                (u,) = free
                true.add(u)     # (-u is not in `true`: u is free)
                changed = True
    return False


def evaluate(formula, proof, max_vars=None):
    """([status, failed, first_failed, flags], lemma_ok) of `proof` against `formula`."""
    if max_vars is None:
        max_vars = max_vars_of(formula, proof)
    flags = 0
    premises = []
    for c in formula:
        if any(_is_bad(l, max_vars) for l in c):
            flags |= BAD_LITERAL
        else:
            premises.append(set(c))
    failed, first, ended = 0, -1, False
    lemma_ok = []
    for i, lemma in enumerate(proof):
        if ended:
            lemma_ok.append(-1)
            continue
        bad = any(_is_bad(l, max_vars) for l in lemma)
        good = {l for l in lemma if not _is_bad(l, max_vars)}
        taut = any(-l in good for l in good)
        if bad:
            flags |= BAD_LITERAL
        if taut:
            flags |= TAUTOLOGY
        ok = not bad and (taut or propagates_to_conflict(premises, {-l for l in good}))
        lemma_ok.append(1 if ok else 0)
        if not ok:
            failed += 1
            if first < 0:
                first = i
        if not bad:
            premises.append(good)
        ended = len(lemma) == 0
    status = FAILED if failed else PROVEN if ended else OPEN
    return [status, failed, first, flags], lemma_ok


def expected(formulas, proofs, max_vars=None):
    """(the [B][4] words, the lemma verdicts of all proofs in one list); max_vars=None: per
    call, over the whole batch (the host form's)."""
    if max_vars is None:
        max_vars = max([max_vars_of(f, p) for f, p in zip(formulas, proofs)] + [0])
    words, oks = [], []
    for f, p in zip(formulas, proofs):
        w, ok = evaluate(f, p, max_vars)
        words.append(w)
        oks += ok
    return words, oks


# ---- brute force (test_refute.py)
def implied(premises, clause, nvars):
    """Whether every total assignment of variables 1 .. nvars that satisfies every clause of
    `premises` satisfies `clause`, by enumeration."""
    for bits in range(1 << nvars):
        val = lambda l: ((bits >> (abs(l) - 1)) & 1) == (l > 0)   # noqa: E731
        if all(any(val(l) for l in c) for c in premises) and not any(val(l) for l in clause):
            return False
    return True


def random_small(seed, count=400, nmax=5):
    """(formula, proof) pairs over at most `nmax` variables: clauses and lemmas of 0 .. 3
    literals (repeats and tautologies included), a few proofs with an empty lemma inside."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(1, nmax)

        def clause(lo):
            return [rng.choice((1, -1)) * rng.randint(1, n) for _ in range(rng.randint(lo, 3))]
        f = [clause(0 if rng.random() < 0.05 else 1) for _ in range(rng.randint(0, 2 * n + 2))]
        p = [clause(0 if rng.random() < 0.2 else 1) for _ in range(rng.randint(0, 6))]
        out.append((f, p))
    return out


# ---- test 1: the edge batch, (formula, proof, want words, want lemma_ok)
QUAD = [[1, 2, 3], [1, 2, -3], [1, -2, 3], [1, -2, -3]]   # implies [1]; no unit propagation gets there
EDGE_CASES = [
    ([[1, 2]], [], [OPEN, 0, -1, 0], []),                                       # an empty proof
    ([[1], [-1]], [[]], [PROVEN, 0, -1, 0], [1]),
    ([[1, 2], [-1, 2]], [[]], [FAILED, 1, 0, 0], [0]),                          # [] on a satisfiable set
    ([], [[1]], [FAILED, 1, 0, 0], [0]),                                        # a formula with no clauses
    ([], [[1, -1], []], [FAILED, 1, 1, TAUTOLOGY], [1, 0]),
    ([[1, 2], []], [[3], []], [PROVEN, 0, -1, 0], [1, 1]),                      # the formula holds the empty clause
    ([[1, -2], [2, 3]], [[1, -2]], [OPEN, 0, -1, 0], [1]),                      # a lemma equal to a formula clause
    ([[1, 2]], [[3, -3]], [OPEN, 0, -1, TAUTOLOGY], [1]),                       # a tautological lemma
    ([[1, 2], [-2]], [[1, 1, 1]], [OPEN, 0, -1, 0], [1]),                       # a lemma with repeated literals
    ([[2, 2], [-2, 1, 1]], [[1]], [OPEN, 0, -1, 0], [1]),                       # ... and clauses with them
    (QUAD, [[1]], [FAILED, 1, 0, 0], [0]),                                      # implied, not verified
    (QUAD, [[1, 2], [1]], [OPEN, 0, -1, 0], [1, 1]),
    ([[1], [-1]], [[2], [], [3], []], [PROVEN, 0, -1, 0], [1, 1, -1, -1]),      # behind the first empty lemma
    ([[1], [-1, 2]], [[], [2], []], [FAILED, 1, 0, 0], [0, -1, -1]),
    ([[-3, 1]], [[3], [1], [-3, 1]], [FAILED, 1, 0, 0], [0, 1, 1]),             # a failed lemma is a premise of the next
    ([[1, 2], [-1, 2], [1, -2], [-1, -2]], [[1], []], [PROVEN, 0, -1, 0], [1, 1]),
]


# ---- test 2: propagation depth
DEPTHS = (1, 2, 64, 65)


def chain_cases(k):
    """The implications x1 -> x2 -> ... -> xk as clauses in reverse order, so that a full
    scan in clause order carries x1 one clause further; the lemma [-1, k] verifies, and
    fails with the chain's last clause [-(k-1), k] missing (for k = 1 the chain has no
    clause and [-1, 1] is a tautology either way).  Its assumption -k runs down the chain
    as well, so a third case has only x1 to start from: the lemma [-1] with xk -> x(k+1)
    and xk -> -x(k+1) behind the chain takes k + 1 assignments, one after the other."""
    chain = [[-v, v + 1] for v in range(k - 1, 0, -1)]
    forward = [[-k, -(k + 1)], [-k, k + 1]] + chain
    return [(chain, [[-1, k]]), (chain[1:], [[-1, k]]), (forward, [[-1]])]


# ---- test 5: counts
CLAUSE_COUNTS = (0, 1, 63, 64, 65, 129)
LEMMA_COUNTS = (1, 63, 64, 65)


def clause_count_case(m):
    """m clauses, the decisive one last: m - 1 clauses [2, 3 + i] that decide nothing and
    [1]; the lemma [1] verifies only through the last (with m = 0 it fails)."""
    return [[2, 3 + i] for i in range(m - 1)] + ([[1]] if m else []), [[1]]


def lemma_count_case(k):
    """The formula [1] and the lemmas [-1, 2], [-2, 3], ...: lemma i = [-(i+1), i+2] fails
    (nothing forces it) and stays a premise, and the last lemma [k] verifies only through
    every lemma before it, the one just before it included -- for k = 1 it is [1] itself."""
    return [[1]], [[-(i + 1), i + 2] for i in range(k - 1)] + [[k]]


# ---- test 6: clause lengths on both sides of the two forms' threshold
CLAUSE_LENGTHS = (1, 2, SHORT_MAX, SHORT_MAX + 1, 64, 65, 300)


def length_case(k):
    """Two (formula, proof) pairs with a clause of k literals whose only unassigned literal
    is its last.  A formula clause: under the assumptions of the lemma [1 .. k-1, k+1] the
    clause [1 .. k] forces k, and [-k, k+1] is the conflict.  A lemma as a premise: the same
    lemma fails against [[-(k+1), k+2]] alone, and under the assumptions of [1 .. k-1, k+2]
    it forces k+1, which that clause turns into the conflict."""
    first = list(range(1, k)) + [k + 1]
    second = list(range(1, k)) + [k + 2]
    return [([list(range(1, k + 1)), [-k, k + 1]], [first]),          # -> [OPEN, 0, -1, 0], [1]
            ([[-(k + 1), k + 2]], [first, second])]                   # -> [FAILED, 1, 0, 0], [0, 1]


def negate_one(proof, rng):
    """`proof` with one literal negated in one non-empty lemma (None if it has none)."""
    spots = [i for i, c in enumerate(proof) if c]
    if not spots:
        return None
    i = rng.choice(spots)
    out = [list(c) for c in proof]
    j = rng.randrange(len(out[i]))
    out[i][j] = -out[i][j]
    return out


def random_3sat(count, n, m, seed):
    """`count` formulas of m clauses of 3 distinct variables of 1 .. n, each negated w.p. 1/2."""
    rng = random.Random(seed)
    return [[[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), 3)] for _ in range(m)]
            for _ in range(count)]
