"""The sound CDCL's search rule under assumptions in plain Python, and the rows of its tests
(tests/test_cdcl_assume_rows.py holds the rule to brute force and to a plain RUP check;
tests/test_cdcl_assume_gpu.py holds the assumption-carrying kernel of csrc/cdcl_sound.hip
to the rule).

The rule is include/satmi.h's (satmi_cdcl_assume_batch_device): cdcl_sound_rows.solve's with
an ordered list of assumption literals a_1 .. a_k.  Level i <= k belongs to a_i: at a fixpoint
below level k the next assumption opens its level (empty when it already holds) or, being
false, ends the search ASSUMED with the core the final analysis collects over the trail.
Free decisions start at level k."""
import random

import cdcl_sound_rows as R
import refute_rows as rr

UNSAT, SAT, LIMIT, FULL, TOO_LARGE, ASSUMED = range(6)
COUNTERS = R.COUNTERS


def solve(formula, assumptions=(), conflict_limit=0, *, halve=R.HALVE):
    """{"status", "counters": [8], "model": signed literals ascending by variable or None,
    "lemmas": the learned clauses in order, [] last when UNSAT or ASSUMED, "core": the failed
    assumptions (ASSUMED), [] (UNSAT) or None, "paths": cdcl_sound_rows.solve's}.  `halve` as
    there."""
    clauses = [list(c) for c in formula]
    assume = list(assumptions)
    k = len(assume)
    occurs = sorted({abs(l) for c in formula for l in c} | {abs(a) for a in assume})
    val, level, reason, trail = {}, {}, {}, []
    act = {v: 0 for v in occurs}
    phase = {v: False for v in occurs}
    n = dict.fromkeys(COUNTERS, 0)
    lemmas = []
    paths = dict.fromkeys(R.PATHS, 0)
    core = None
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
                    return i
                if len(free) == 1:
                    (u,) = free
                    paths["opposite offers lost"] += abs(u) in units and units[abs(u)][1] == -u
                    units.setdefault(abs(u), (i, u))
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

    def final(a):
        """The assumptions that made `a` false: `a`, then those reached from it through the
        reasons, in descending trail position."""
        out, seen = [a], set()
        if level[abs(a)] > 0:
            seen.add(abs(a))
        gap = 0
        for l in reversed(trail):
            v = abs(l)
            if level[v] == 0:
                break
            if v not in seen:
                gap += 1
                continue
            paths["final walk gap"], gap = max(paths["final walk gap"], gap), 0
            if reason[v] is None:
                out.append(l)
            else:
                seen.update(abs(q) for q in clauses[reason[v]] if abs(q) != v and level[abs(q)] > 0)
        return out

    while True:
        confl = propagate()
        if confl is not None:
            n["conflicts"] += 1
            if cur == 0:
                lemmas.append([])
                status, core = UNSAT, []
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
        if cur < k:     # the next assumption's level
            a = assume[cur]
            if value(a) is False:
                core = final(a)
                lemmas.append([])
                status = ASSUMED
                break
            cur += 1
            n["max_level"] = max(n["max_level"], cur)
            if value(a) is None:
                val[abs(a)], level[abs(a)], reason[abs(a)] = a > 0, cur, None
                trail.append(a)
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
    return {"status": status, "counters": [n[c] for c in COUNTERS],
            "model": [v if val[v] else -v for v in occurs] if status == SAT else None, "lemmas": lemmas,
            "core": core, "paths": paths}


def rup(clauses, lemma):
    """Whether assigning `lemma`'s literals false and propagating units over `clauses` to a
    fixpoint reaches a conflict (plain reverse unit propagation)."""
    true = {-l for l in lemma}
    if any(-l in true for l in true):
        return True
    while True:
        grew = False
        for c in clauses:
            if any(l in true for l in c):
                continue
            free = {l for l in c if -l not in true}
            if not free:
                return True
            if len(free) == 1:
                true |= free
                grew = True
        if not grew:
            return False


def refutes(formula, lemmas):
    """Every lemma is RUP from `formula` and the lemmas before it, and the last is empty."""
    db = [list(c) for c in formula]
    for c in lemmas:
        if not rup(db, c):
            return False
        db.append(list(c))
    return bool(lemmas) and lemmas[-1] == []


def is_sublist(core, assumptions):
    """Every literal of the core is one of the assumptions, and none is repeated."""
    return len(set(core)) == len(core) and set(core) <= set(assumptions)


def random_assumptions(rng, nv, extra=True):
    """0 .. 4 assumption literals over 1 .. nv, one of them possibly over nv + 1."""
    out = [rng.choice((1, -1)) * rng.randint(1, nv) for _ in range(rng.randint(0, 4))]
    if extra and out and rng.random() < 0.2:
        out[rng.randrange(len(out))] = rng.choice((1, -1)) * (nv + 1)
    return out


# ---- the rows
def chain_row(n):
    """The single clause [-1 .. -n] under 1 .. n: the first n - 1 assumptions make it unit, and
    the last is false by it; the core is all n, n .. 1."""
    return [[-v for v in range(1, n + 1)]], list(range(1, n + 1))


SELECTORS = list(range(13, 19))


def php_selector_row(selectors=SELECTORS):
    """PHP(3), every clause carrying one of six negated selectors 13 .. 18 in turn, under
    20, 21, the selectors given, 22: with all six the formula is PHP(3), with five a clause
    group is switched off."""
    f = [c + [-SELECTORS[i % 6]] for i, c in enumerate(R.php(3))]
    return f, [20, 21] + list(selectors) + [22]


RANDOM_SEED, RANDOM_COUNT = 20262, 64


def random_row(seed=RANDOM_SEED):
    """cdcl_sound_rows' kind of random 3-SAT, formula i under i % 4 random assumptions over
    distinct variables."""
    rng = random.Random(seed)
    fs = rr.random_3sat(RANDOM_COUNT, 50, 213, seed)
    return [(f, [rng.choice((1, -1)) * v for v in rng.sample(range(1, 51), i % 4)]) for i, f in enumerate(fs)]


def rows():
    """(name, formula, assumptions) triples: every row of the kernel's parity test."""
    out = [(n, f, []) for n, f in R.rows()]
    out += [
        ("unit against its assumption", [[1]], [-1]),
        ("contradicting assumptions", [[1, 2]], [3, 3, -3]),
        ("empty levels and a new variable", [[1, 2]], [1, 1, 5]),
        ("php 3 under six selectors",) + php_selector_row(),
        ("php 3 under five selectors",) + php_selector_row(SELECTORS[:5]),
        ("unit lemma through two assumption levels", [[1, 2], [1, -2], [-1, 3], [-1, -3, 4]], [5, 6]),
    ]
    out += [(f"chain of {n}",) + chain_row(n) for n in (1, 2, 64, 65)]
    out += [(f"random 3-SAT {i} assumed", f, a) for i, (f, a) in enumerate(random_row())]
    return out
