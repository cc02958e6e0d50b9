"""The sound CDCL's search rule in plain Python, and the rows of its tests
(tests/test_cdcl_sound_rows.py holds the rule to brute force and to the oracle;
tests/test_cdcl_sound_gpu.py holds the kernel of csrc/cdcl_sound.hip to the rule).

The rule is include/satmi.h's (satmi_cdcl_sound_batch_device): rounds of unit
propagation over formula and learned clauses under the assignment of the round's
start, the lowest-indexed falsified clause as the conflict, the lowest-indexed
unit clause as a variable's reason, first-UIP learning with level-0 literals
dropped, integer activities halved every 256 conflicts, saved phases, no restarts.

solve also reports which structural paths of the kernel the search went down (PATHS), and
takes another halving than the rule's by keyword: both for tests/cdcl_sound_paths.py."""
import random

import refute_rows as rr

UNSAT, SAT, LIMIT, FULL, TOO_LARGE = range(5)
COUNTERS = ("conflicts", "decisions", "propagated", "rounds", "learned", "learned_literals", "max_level", "restarts")
MAX_VARS = 8191      # SATMI_CDCL_SOUND_MAX_VARS
SHORT_MAX = 8        # csrc/cdcl_sound.hip's CS_SHORT_MAX: the longest clause of the lane-per-clause form


PATHS = ("halvings", "decisions past lane 63 by activity", "first-UIP walk gap", "collection walk gap",
         "final walk gap", "deepest level", "opposite offers lost")
HALVE = (256, 0, 0)     # the rule's halving: when conflicts % 256 == 0, rounding down
# what is not the rule (tests/test_cdcl_sound_paths.py: every halving row tells each from it)
NOT_THE_RULE = {"no halving": (0, 0, 0), "one conflict early": (256, 255, 0), "rounding up": (256, 0, 1)}


def solve(formula, conflict_limit=0, *, halve=HALVE):
    """{"status", "counters": [8], "model": signed literals ascending by variable or None,
    "lemmas": the learned clauses in order, [] last when UNSAT, "paths": how often, or how
    far, the search went down each of PATHS (tests/cdcl_sound_paths.py)}.  `halve` = (period,
    remainder, 1 to round up): another than HALVE is another rule."""
    clauses = [list(c) for c in formula]
    occurs = sorted({abs(l) for c in formula for l in c})
    val, level, reason, trail = {}, {}, {}, []
    act = {v: 0 for v in occurs}
    phase = {v: False for v in occurs}
    n = dict.fromkeys(COUNTERS, 0)
    lemmas = []
    paths = dict.fromkeys(PATHS, 0)
    cur = 0

    def value(l):
        return None if abs(l) not in val else val[abs(l)] == (l > 0)

    def propagate():
        """The index of the conflict clause, or None at the fixpoint."""
        while True:
            n["rounds"] += 1
            units = {}
            for i, c in enumerate(clauses):
                vals = [value(l) for l in c]
                if True in vals:
                    continue
                free = {l for l, x in zip(c, vals) if x is None}
                if not free:
                    return i          # the lowest-indexed falsified clause; the round implies nothing
                if len(free) == 1:
                    (u,) = free
                    paths["opposite offers lost"] += abs(u) in units and units[abs(u)][1] == -u
                    units.setdefault(abs(u), (i, u))   # the lowest-indexed clause that implies the variable
            if not units:
                return None
            for i, u in sorted(units.values()):
                val[abs(u)], level[abs(u)], reason[abs(u)] = u > 0, cur, i
                trail.append(u)
                n["propagated"] += 1

    def analyze(confl):
        seen, count, c, pvar, idx = set(), 0, clauses[confl], None, len(trail) - 1
        while True:
            for q in c:
                v = abs(q)
                if v != pvar and v not in seen and level[v] > 0:
                    seen.add(v)
                    count += level[v] == cur
            top = idx
            while abs(trail[idx]) not in seen:
                idx -= 1
            paths["first-UIP walk gap"] = max(paths["first-UIP walk gap"], top - idx)
            p = trail[idx]
            pvar = abs(p)
            seen.discard(pvar)
            idx -= 1
            count -= 1
            if count == 0:
                break
            c = clauses[reason[pvar]]
        low = [i for i in range(idx, -1, -1) if abs(trail[i]) in seen]
        if low:
            paths["collection walk gap"] = max(paths["collection walk gap"], idx - low[0])
        return [-p] + [-trail[i] for i in low]

    while True:
        confl = propagate()
        if confl is not None:
            n["conflicts"] += 1
            if cur == 0:
                lemmas.append([])
                status = UNSAT
                break
            if conflict_limit > 0 and n["conflicts"] >= conflict_limit:
                status = LIMIT
                break
            lemma = analyze(confl)
            clauses.append(lemma)
            lemmas.append(lemma)
            n["learned"] += 1
            n["learned_literals"] += len(lemma)
            for l in lemma:
                act[abs(l)] += 1
            cur = max([level[abs(l)] for l in lemma[1:]] + [0])
            while trail and level[abs(trail[-1])] > cur:
                v = abs(trail.pop())
                phase[v] = val.pop(v)
            if halve[0] and n["conflicts"] % halve[0] == halve[1]:
                paths["halvings"] += 1
                for v in act:
                    act[v] = (act[v] + halve[2]) // 2
            continue
        cands = [v for v in occurs if v not in val]
        if not cands:
            status = SAT
            break
        v = max(cands, key=lambda x: (act[x], -x))
        paths["decisions past lane 63 by activity"] += v > 64 and v != cands[0]
        cur += 1
        n["decisions"] += 1
        n["max_level"] = max(n["max_level"], cur)
        val[v], level[v], reason[v] = phase[v], cur, None
        trail.append(v if phase[v] else -v)
    paths["deepest level"] = n["max_level"]
    return {"status": status, "counters": [n[k] for k in COUNTERS],
            "model": [v if val[v] else -v for v in occurs] if status == SAT else None, "lemmas": lemmas,
            "paths": paths}


def region_words(lemmas):
    """Words of the records `len, lit_1 .. lit_len` of a lemma list."""
    return sum(1 + len(c) for c in lemmas)


def satisfies(formula, model):
    true = set(model)
    return all(any(l in true for l in c) for c in formula)


def brute_force(formula):
    vs = sorted({abs(l) for c in formula for l in c})
    for bits in range(1 << len(vs)):
        true = {v if (bits >> i) & 1 else -v for i, v in enumerate(vs)}
        if all(any(l in true for l in c) for c in formula):
            return True
    return False


def random_small(seed, count):
    """Formulas over at most 8 variables: clauses of 0 .. 4 literals, repeats and tautologies included."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        nv = rng.randint(1, 8)
        m = rng.randint(0, 5 * nv)
        lo = 0 if rng.random() < 0.03 else 1
        out.append([[rng.choice((1, -1)) * rng.randint(1, nv) for _ in range(rng.randint(lo, 4))] for _ in range(m)])
    return out


# ---- the rows
def php(holes):
    """holes + 1 pigeons into `holes` holes: UNSAT, and no short refutation by unit propagation."""
    x = lambda p, h: p * holes + h + 1   # noqa: E731
    f = [[x(p, h) for h in range(holes)] for p in range(holes + 1)]
    f += [[-x(p, h), -x(q, h)] for h in range(holes) for p in range(holes + 1) for q in range(p + 1, holes + 1)]
    return f


def learned_length_row(k):
    """A formula whose first learned clause has k literals (k >= 2): the decisions -1 .. -(k-1)
    fall in id order, level by level, with nothing implied; deciding -k implies y = k + 1 through
    [k, y] and the clause [1 .. k, -y] is falsified.  The first UIP is -k itself, and the clause
    learned is [k, k-1 .. 1].  Every clause but the first has k + 1 literals."""
    y = k + 1
    return [[k, y], list(range(1, k + 1)) + [-y]]


def clause_count_row(m):
    """m clauses, the decisive pair last: the fillers [2, 3 + i] force nothing until [1] and
    [-1, -2] have implied -2, two rounds later; the third round finds every filler unit, m - 2
    implied variables across the 64-clause steps."""
    return [[2, 3 + i] for i in range(m - 2)] + [[1], [-1, -2]]


def long_clause_row(k=300):
    """A clause of k literals beside short ones: the launch takes the wave-per-clause form.
    Deciding -1 implies -3, -k and then -2; the variables 4 .. k-2 are decided False one by
    one, and the long clause, every other literal false, then implies k-1."""
    return [list(range(1, k + 1)), [-k, 1], [-k, 2, 3], [-2, 3], [-3, 1]]


def sparse_row(top=MAX_VARS):
    """A handful of variables next to the variable limit: an UNSAT core over top-3 .. top that
    needs learning, beside a satisfiable clause over small ids."""
    a, b, c = top - 2, top - 1, top
    quad = [[a, b, c], [a, b, -c], [a, -b, c], [a, -b, -c]]
    return quad + [[-a, 5], [-a, -5, 7], [-a, -7]]


RANDOM_SEED, RANDOM_COUNT = 20261, 64      # test_cdcl_sound_rows.py: at least 8 SAT and 8 UNSAT by the oracle


def random_row():
    return rr.random_3sat(RANDOM_COUNT, 50, 213, RANDOM_SEED)


def rows():
    """(name, formula) pairs: every row of the kernel's parity test."""
    out = [
        ("empty formula", []),
        ("empty clause", [[]]),
        ("opposite units", [[1], [-1]]),
        ("quad needs learning", rr.QUAD + [[-1]]),
        ("first learned clause is a unit", [[1, 2], [1, -2], [-1, 3], [-1, -3]]),
        ("repeated literals", [[2, 2, 1], [-2, -2, 1, 1], [-1, -1, 3, 3], [-1, -3, -3]]),
        ("tautologies", [[1, -1], [2, -2, 3], [-3, 1], [-1, 3, -3], [-1, -2], [2, 1]]),
        ("tautology only", [[4, -4]]),
        ("sparse ids", sparse_row()),
        ("php 3", php(3)),
        ("php 4", php(4)),
        ("long clause", long_clause_row()),
    ]
    out += [(f"learned clause of {k}", learned_length_row(k)) for k in (2, 8, 9, 64, 65)]
    out += [(f"{m} clauses", clause_count_row(m)) for m in (63, 64, 65, 129)]
    out += [(f"random 3-SAT {i}", f) for i, f in enumerate(random_row())]
    return out
