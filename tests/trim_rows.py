"""The refutation trim's rule in plain Python, the properties every answer to it
must have, and the hand-built rows of its tests (tests/test_trim.py holds the
Python trimmer to brute force; tests/test_trim_gpu.py holds the kernel to the
same properties and, where the answer is unique, to the rows' marks).

The trim walks a proof backwards from its first empty lemma and checks only the
lemmas that lemma needs, as tests/refute_rows.py checks them; every propagated
literal remembers the clause that made it unit, and a conflict marks its
clause(s) and, transitively, the reason of every false literal of a marked
clause.  Which clauses that is depends on the propagation order, so the trimmer
below is no oracle for the marks: it takes the order as an argument, and what
the tests hold any trimmer to are the properties of `check_properties`."""
import random

import refute_rows as rr

MAX_VARS = 16383     # SATMI_TRIM_MAX_VARS
NWORDS = 6           # status, failed, first_failed, flags, core clauses, kept lemmas


def _propagate(premises, assumed, rng):
    """Unit propagation over `premises` ([(id, set of literals)]) from the true literals
    `assumed`: None at a fixpoint, else the set of premise ids the conflict rests on -- the
    falsified clause and, transitively, the reason of each of a marked clause's false literals.
    One clause at a time; `rng` (or None) shuffles the clause order of every round."""
    true = set(assumed)
    reason = {}
    conflict = None
    changed = True
    while changed and conflict is None:
        changed = False
        order = list(premises)
        if rng is not None:
            rng.shuffle(order)
        for cid, c in order:
            if any(l in true for l in c):
                continue
            free = {l for l in c if -l not in true}
            if not free:
                conflict = cid
                break
            if len(free) == 1:
                (u,) = free
                true.add(u)
                reason[u] = cid
                changed = True
    if conflict is None:
        return None
    clauses = dict(premises)
    marked, todo = set(), [conflict]
    while todo:
        cid = todo.pop()
        if cid in marked:
            continue
        marked.add(cid)
        todo += [reason[-l] for l in clauses[cid] if -l in reason]
    return marked


def trim(formula, proof, max_vars=None, rng=None):
    """([status, failed, first_failed, flags, core clauses, kept lemmas], core marks, lemma marks)."""
    if max_vars is None:
        max_vars = rr.max_vars_of(formula, proof)
    m, k = len(formula), len(proof)
    core, lemma = [0] * m, [-1] * k
    bad = lambda c: any(rr._is_bad(l, max_vars) for l in c)   # noqa: E731
    flags = rr.BAD_LITERAL if any(bad(c) for c in formula) else 0
    end = next((i for i, c in enumerate(proof) if not c), None)
    if end is None:
        return [rr.OPEN, 0, -1, flags, 0, 0], core, lemma
    lemma[end] = 1
    failed, first = 0, -1
    for i in range(end, -1, -1):
        if lemma[i] < 0:
            continue
        good = {l for l in proof[i] if not rr._is_bad(l, max_vars)}
        taut = any(-l in good for l in good)
        if bad(proof[i]):
            flags |= rr.BAD_LITERAL
        if taut:
            flags |= rr.TAUTOLOGY
        marked = None
        if not bad(proof[i]) and not taut:
            premises = [(c, set(formula[c])) for c in range(m) if not bad(formula[c])]
            premises += [(m + j, set(proof[j])) for j in range(i) if not bad(proof[j])]
            marked = _propagate(premises, {-l for l in good}, rng)
        if bad(proof[i]) or (marked is None and not taut):
            lemma[i] = 0
            failed += 1
            first = i
        for cid in marked or ():
            if cid < m:
                core[cid] = 1
            else:
                lemma[cid - m] = 1
    status = rr.FAILED if failed else rr.PROVEN
    return [status, failed, first, flags, sum(core), sum(x >= 0 for x in lemma)], core, lemma


def check_properties(formula, proof, words, core, lemma, max_vars=None, brute_nvars=None):
    """Assert what any valid trim of (formula, proof) satisfies; `words`, `core`, `lemma` are one
    instance's.  brute_nvars: also hold a PROVEN core to enumeration over that many variables."""
    if max_vars is None:
        max_vars = rr.max_vars_of(formula, proof)
    words, core, lemma = list(words), list(core), list(lemma)
    assert len(words) == NWORDS and len(core) == len(formula) and len(lemma) == len(proof)
    status, failed, first = words[:3]
    fwd, fwd_ok = rr.evaluate(formula, proof, max_vars)
    end = next((i for i, c in enumerate(proof) if not c), None)
    assert set(core) <= {0, 1} and set(lemma) <= {-1, 0, 1}
    assert words[4] == sum(core) and words[5] == sum(x >= 0 for x in lemma)   # the words are the marks' sums
    assert failed == lemma.count(0)
    formula_bad = rr.BAD_LITERAL if any(rr._is_bad(l, max_vars) for c in formula for l in c) else 0
    assert words[3] & ~fwd[3] == 0 and words[3] & formula_bad == formula_bad   # needed lemmas are checked ones
    if end is None:                                         # no empty lemma: OPEN, nothing marked
        assert words == [rr.OPEN, 0, -1, words[3], 0, 0] and not any(core) and set(lemma) <= {-1}
        return
    assert status in (rr.FAILED, rr.PROVEN)
    assert all(x == -1 for x in lemma[end + 1:])            # behind the ending lemma: never looked at
    assert lemma[end] >= 0                                  # the ending lemma is needed
    assert (status == rr.FAILED) == (failed > 0)
    if fwd[0] == rr.PROVEN:                                 # forward PROVEN => trim PROVEN
        assert status == rr.PROVEN
    if status == rr.FAILED:                                 # trim FAILED => forward FAILED
        assert fwd[0] == rr.FAILED
        assert first == lemma.index(0) and fwd_ok[first] == 0
        assert all(fwd_ok[i] == 0 for i, x in enumerate(lemma) if x == 0)
    else:
        assert first == -1 and lemma[end] == 1
        core_clauses = [formula[c] for c in range(len(formula)) if core[c]]
        kept = [proof[j] for j in range(len(proof)) if lemma[j] >= 0]
        assert kept[-1] == []
        got, _ = rr.evaluate(core_clauses, kept, max_vars)  # PROVEN => the forward check accepts core + kept
        assert got[:3] == [rr.PROVEN, 0, -1], (core_clauses, kept, got)
        if brute_nvars is not None:
            assert rr.implied(core_clauses, [], brute_nvars)


def split(words, core, lemma, formulas, proofs):
    """A batch's flat outputs -> [(words, core marks, lemma marks)] per instance."""
    out, c, p = [], 0, 0
    for b, (f, pr) in enumerate(zip(formulas, proofs)):
        out.append((list(words[b]), list(core[c:c + len(f)]), list(lemma[p:p + len(pr)])))
        c += len(f)
        p += len(pr)
    return out


# ---- rows whose answer is unique: (formula, proof, status, core indices, kept indices)
XOR2 = [[1, 2], [-1, 2], [1, -2], [-1, -2]]
LADDERS = (1, 62, 63, 64, 65)   # k + 1 lemmas: 2, and 63 .. 66


def lemma_ladder(k):
    """Variables y0 .. yk (1 .. k + 1), a1 .. ak, z.  The formula: [y0]; per rung j the clauses
    [-y(j-1), aj, yj] and [-y(j-1), -aj, yj]; [-yk, z] and [-yk, -z].  The proof: [y1], .., [yk], [].
    Unit propagation from the formula alone stops at y0.  [] gets yk only from the lemma [yk]
    and then needs z with both signs; [yj] gets y(j-1) only from the lemma before it (rung j's
    clauses have two open literals until then) and then needs aj with both signs.  So whatever the
    order, every clause is in the core and every lemma is needed, each through the one behind it."""
    a = lambda j: k + 1 + j   # noqa: E731
    z = 2 * k + 2
    f = [[1]]
    for j in range(1, k + 1):
        f += [[-j, a(j), j + 1], [-j, -a(j), j + 1]]
    f += [[-(k + 1), z], [-(k + 1), -z]]
    return f, [[j + 1] for j in range(1, k + 1)] + [[]]


def unique_rows():
    rows = []
    # two opposite units among 50 clauses over other variables
    rows.append(([[1], [-1]] + [[2 + i, 3 + i] for i in range(50)], [[]], rr.PROVEN, [0, 1], [0]))
    # forward FAILED at lemma 0, which nothing needs; [3, 4] is not in the core
    rows.append((XOR2 + [[3, 4]], [[5, 6], [2], []], rr.PROVEN, [0, 1, 2, 3], [1, 2]))
    # unit chains: every clause is in the core (the trail walk across the 64-entry boundary)
    for k in rr.DEPTHS:
        f = [[1]] + [[-v, v + 1] for v in range(1, k)] + [[-k]]
        rows.append((f, [[]], rr.PROVEN, list(range(len(f))), [0]))
    # lemma ladders: marking lemmas through lemmas, every lemma needed and verified
    for k in LADDERS:
        f, p = lemma_ladder(k)
        rows.append((f, p, rr.PROVEN, list(range(len(f))), list(range(len(p)))))
    # the forward check's edge cases that hold [] and have one answer
    rows.append(([[1], [-1]], [[]], rr.PROVEN, [0, 1], [0]))
    rows.append(([[1, 2], [-1, 2]], [[]], rr.FAILED, [], [0]))
    rows.append(([[1, 2], []], [[3], []], rr.PROVEN, [1], [1]))
    rows.append(([[1], [-1]], [[2], [], [3], []], rr.PROVEN, [0, 1], [1]))
    rows.append(([[1], [-1, 2]], [[], [2], []], rr.FAILED, [], [0]))
    rows.append(([], [[1, -1], []], rr.FAILED, [], [1]))
    return rows


def lemma_chain_through_failed(k):
    """refute_rows.lemma_count_case(k) closed: the formula [1], [-k] and the lemmas [-1, 2],
    [-2, 3], ... (none verifies, each stays a premise), [k] and []: [] needs [k] and [-k]; [k]
    verifies through every lemma before it, marks them all needed, and each of them fails."""
    f, p = rr.lemma_count_case(k)
    return f + [[-k]], p + [[]]


def counts_rows():
    """CLAUSE_COUNTS and LEMMA_COUNTS, each closed with what reaches []: properties only."""
    rows = []
    for m in rr.CLAUSE_COUNTS:
        f, p = rr.clause_count_case(m)
        rows.append((f + [[-1]], p + [[]]))
    for k in rr.LEMMA_COUNTS:
        rows.append(lemma_chain_through_failed(k))
    return rows


def length_rows(k):
    """refute_rows.length_case(k), each pair closed: the first with [-(k+1)] and [], the second
    (whose first lemma fails forwards) with [-(k+2)] and []."""
    (f1, p1), (f2, p2) = rr.length_case(k)
    units = [[-v] for v in range(1, k)]   # the lemmas' other literals, refuted one by one
    return [(f1 + units + [[-(k + 1)]], p1 + [[]]), (f2 + units + [[-(k + 2)]], p2 + [[]])]


# ---- reuse: 40 instances through one wave, (formula, proof, core indices, kept indices)
# over variables 1 .. 5; the lemma [2] and then [] each need both halves of XOR2
REUSE_A = (XOR2 + [[3, 4], [-3, 5]], [[2], []], [0, 1, 2, 3], [0, 1])
# 3 -> 4 -> 5 against [-4, -5]: every variable ends up assigned and on the conflict side, each with
# a reason.  With 3 left true in the table from the instance before, [3] would be satisfied, not
# a reason, and clause 0 would be missing from the core.
REUSE_B = ([[3], [-3, 4], [-4, 5], [3, 6], [-4, -5]], [[]], [0, 1, 2, 4], [0])
# 3 and 2 are assigned in the first round, by clauses 0 and 1; the conflict of the second round
# is about 2 alone.  With 3 left on the conflict side from the instance before, its reason [3]
# would be marked and clause 0 would join the core.
REUSE_D = ([[3], [2], [-2, 1], [-2, -1]], [[]], [1, 2, 3], [0])


def reuse_rows():
    return [REUSE_B, REUSE_D, REUSE_A, REUSE_D] * 10


def random_rows(seeds=range(5), count=400):
    """refute_rows.random_small pairs as they are and with [] appended."""
    rows = []
    for seed in seeds:
        for f, p in rr.random_small(seed, count=count):
            rows.append((f, p))
            rows.append((f, p + [[]]))
    return rows


def rng_orders():
    return [None, random.Random(1), random.Random(2)]
