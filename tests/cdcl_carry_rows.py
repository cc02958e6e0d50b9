"""The sound CDCL's search rule with carried lemmas in plain Python, and the rows of its tests
(tests/test_cdcl_carry_rows.py holds the rule to brute force and to a plain RUP check;
tests/test_cdcl_carry_gpu.py holds the carrying kernel of csrc/cdcl_sound.hip to the rule).

The rule is include/satmi.h's (satmi_cdcl_carry_batch_device): cdcl_assume_rows.solve's, where
the instance starts with p carried lemmas, clauses the caller asserts to follow from F.  They
are the learned clauses m+0 .. m+p-1, and what this call learns follows them.  From the first
round on they are evaluated, offer units, become conflicts and serve as reasons as learned
clauses do, and their variables occur.  Activities, phases and every counter start afresh:
a resumed search is a restart from level 0 with its lemmas kept."""
import random

import cdcl_assume_rows as A
import cdcl_sound_rows as R
import refute_rows as rr

UNSAT, SAT, LIMIT, FULL, TOO_LARGE, ASSUMED = range(6)
COUNTERS = R.COUNTERS
TRUNCATED, BAD_CARRY = 1, 2     # SATMI_CDCL_SOUND_TRUNCATED, SATMI_CDCL_SOUND_BAD_CARRY
I32_MIN = -(2 ** 31)
HITS = ("carried unit at level 0 in round 1", "carried conflict clause", "carried clause resolved on",
        "carried clause in the final analysis", "carried set refutes at level 0")


def records(lemmas):
    """The region's words for a lemma list: `len, lit_1 .. lit_len` each."""
    out = []
    for c in lemmas:
        out += [len(c)] + list(c)
    return out


def solve(formula, assumptions=(), conflict_limit=0, carry=(), room=None, nvars=None, *, halve=R.HALVE,
          conflicts_before=0):
    """cdcl_assume_rows.solve's dict, where "lemmas" is the region's record list (the carried
    lemmas first, then those learned and written, [] last when UNSAT or ASSUMED), and with it
    "kept" (the non-empty records of the region: what the next query carries), "records" and
    "words" (info[0], info[1]: the closing record and a record that did not fit included),
    "flags" and "hits" (how often each of HITS occurred).  `room` = the region's words (None =
    as many as needed), `nvars` = inst_nvars (None = the largest variable anywhere).  `halve` as in cdcl_sound_rows.solve;
    a `conflicts_before` other than 0 is another rule: the halving keyed on a count that goes on
    from the queries before."""
    clauses = [list(c) for c in formula]
    assume = list(assumptions)
    carried = [list(c) for c in carry]
    m, p, k = len(clauses), len(carried), len(assume)
    hits = dict.fromkeys(HITS, 0)
    paths = dict.fromkeys(R.PATHS, 0)
    top = max([abs(l) for c in clauses + carried for l in c] + [abs(a) for a in assume] + [0])
    nv = top if nvars is None else nvars

    def ended(status, flags, kept):
        return {"status": status, "counters": [0] * len(COUNTERS), "model": None, "lemmas": [], "core": None,
                "kept": kept, "records": 0, "words": 0, "flags": flags, "hits": hits, "paths": paths}

    def beyond(l):
        return l == 0 or l == I32_MIN or abs(l) > nv
    # the instance must fit the layout; then its carry must be well formed
    if nv > R.MAX_VARS or k > R.MAX_VARS or any(beyond(l) for c in clauses for l in c) or any(beyond(a) for a in assume):
        return ended(TOO_LARGE, 0, carried)
    used = R.region_words(carried)
    if (room is not None and used > room) or any(not c or any(beyond(l) for l in c) for c in carried):
        return ended(TOO_LARGE, BAD_CARRY, [])
    clauses += carried
    occurs = sorted({abs(l) for c in clauses for l in c} | {abs(a) for a in assume})
    val, level, reason, trail = {}, {}, {}, []
    act = {v: 0 for v in occurs}
    phase = {v: False for v in occurs}
    n = dict.fromkeys(COUNTERS, 0)
    lemmas = list(carried)
    nrec, nwords = p, used
    core = None
    cur = 0

    def is_carried(i):
        return i is not None and m <= i < m + p

    def fits(words):
        return room is None or used + words <= room

    def value(l):
        return None if abs(l) not in val else val[abs(l)] == (l > 0)

    def propagate():
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
                hits[HITS[0]] += is_carried(i) and cur == 0 and n["rounds"] == 1

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
            q = trail[idx]
            pvar = abs(q)
            seen.discard(pvar)
            idx -= 1
            count -= 1
            if count == 0:
                break
            c = clauses[reason[pvar]]
            hits[HITS[2]] += is_carried(reason[pvar])
        low = [i for i in range(idx, -1, -1) if abs(trail[i]) in seen]
        if low:
            paths["collection walk gap"] = max(paths["collection walk gap"], idx - low[0])
        return [-q] + [-trail[i] for i in low]

    def final(a):
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
                hits[HITS[3]] += is_carried(reason[v])
        return out

    while True:
        confl = propagate()
        if confl is not None:
            n["conflicts"] += 1
            hits[HITS[1]] += is_carried(confl)
            if cur == 0:
                nrec, nwords = nrec + 1, nwords + 1
                if not fits(1):
                    status = FULL
                    break
                lemmas.append([])
                used += 1
                status, core = UNSAT, []
                hits[HITS[4]] += n["learned"] == 0 and (is_carried(confl) or any(map(is_carried, reason.values())))
                break
            if conflict_limit > 0 and n["conflicts"] >= conflict_limit:
                status = LIMIT
                break
            lemma = analyze(confl)
            nrec, nwords = nrec + 1, nwords + 1 + len(lemma)
            if not fits(1 + len(lemma)):
                status = FULL
                break
            clauses.append(lemma)
            lemmas.append(lemma)
            used += 1 + len(lemma)
            n["learned"] += 1
            n["learned_literals"] += len(lemma)
            for l in lemma:
                act[abs(l)] += 1
            cur = max([level[abs(l)] for l in lemma[1:]] + [0])
            while trail and level[abs(trail[-1])] > cur:
                v = abs(trail.pop())
                phase[v] = val.pop(v)
            if halve[0] and (conflicts_before + n["conflicts"]) % halve[0] == halve[1]:
                paths["halvings"] += 1
                for v in act:
                    act[v] = (act[v] + halve[2]) // 2
            continue
        if cur < k:     # the next assumption's level
            a = assume[cur]
            if value(a) is False:
                nrec, nwords = nrec + 1, nwords + 1
                if not fits(1):
                    status = FULL
                    break
                core = final(a)
                lemmas.append([])
                used += 1
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
            "core": core, "kept": [c for c in lemmas if c], "records": nrec, "words": nwords,
            "flags": TRUNCATED if status == FULL else 0, "hits": hits, "paths": paths}


def chain(queries, conflict_limit=0):
    """Queries (formula, assumptions) in turn, each carrying the one before's kept list."""
    out, kept = [], []
    for f, a in queries:
        out.append(solve(f, a, conflict_limit, kept))
        kept = out[-1]["kept"]
    return out


def resume(formula, assumptions=(), conflict_limit=8, most=10000):
    """The search in slices of `conflict_limit` conflicts, each resumed from the kept list, until
    it ends otherwise: (the last result, the number of slices)."""
    kept = []
    for i in range(most):
        r = solve(formula, assumptions, conflict_limit, kept)
        if r["status"] != LIMIT:
            return r, i + 1
        kept = r["kept"]
    raise AssertionError("the resumed search did not end")


# ---- the rows
def random_chain(rng, n=None):
    """(F_0, a_0), (F_1, a_1), ...: 3 .. 5 queries on a seeded random 3-SAT formula over n <= 12
    variables under random assumptions, clauses added between some of them."""
    n = n or rng.randint(6, 12)
    clause = lambda: [rng.choice((1, -1)) * v for v in rng.sample(range(1, n + 1), 3)]   # noqa: E731
    f = [clause() for _ in range(int(rng.uniform(3.0, 5.5) * n))]
    out = []
    for _ in range(rng.randint(3, 5)):
        if out and rng.random() < 0.5:
            f = f + [clause() for _ in range(rng.randint(1, 3))]
        out.append((f, [rng.choice((1, -1)) * rng.randint(1, n) for _ in range(rng.randint(0, 4))]))
    return out


CHAIN_SEED, CHAIN_COUNT = 0xCA22, 300


def random_chains(seed=CHAIN_SEED, count=CHAIN_COUNT):
    rng = random.Random(seed)
    return [random_chain(rng) for _ in range(count)]


def wide_carry_row(k):
    """A carried lemma of k literals over 1 .. k beside the units [-1] .. [-(k-1)]: after one
    round the lemma is unit and implies k, its last literal, across the wave steps."""
    return [[-v] for v in range(1, k)] + [[k, k + 1]], [], [list(range(1, k + 1))]


def rows():
    """(name, formula, assumptions, carry, room, nvars) tuples: every row of the kernel's parity
    test.  The carried lists are lemma lists of earlier queries on the same formula or a
    subset of it, but for the rows named bogus."""
    php3, php4 = R.php(3), R.php(4)
    sel_f, sel_a = A.php_selector_row()
    out = [(n, f, a, [], None, None) for n, f, a in A.rows() if not n.startswith("random 3-SAT")]
    php3_kept = solve(php3)["kept"]
    php4_part = solve(php4, (), 4)["kept"]
    sel_kept = solve(sel_f, sel_a)["kept"]
    sel_part = solve(sel_f, sel_a, 3)["kept"]
    quad = rr.QUAD + [[-1]]
    out += [
        ("carried unit at level 0", [[1, 2], [1, -2], [-1, 3]], [], [[1]], None, None),
        ("carried lemmas refute php 3 at level 0", php3, [], php3_kept, None, None),
        ("php 4 resumed after 4 conflicts", php4, [], php4_part, None, None),
        ("php 4 resumed under assumptions", php4, [1, 6, 11], php4_part, None, None),
        ("php 3 selectors again with every lemma", sel_f, sel_a, sel_kept, None, None),
        ("php 3 selectors resumed after 3 conflicts", sel_f, sel_a, sel_part, None, None),
        ("php 3 five selectors with the six's lemmas", sel_f, A.php_selector_row(A.SELECTORS[:5])[1], sel_kept, None, None),
        ("carried clause implies against an assumption", [[1, 2]], [-2, 3], [[2, -3]], None, None),
        ("carried clause over a new variable", [[1, 2]], [], [[7, -1], [7, 1]], None, None),
        ("carried clause with repeats and a tautology", [[1, 2], [-1, 2]], [], [[2, 2, 1], [3, -3, 1]], None, None),
        ("carried reason under assumptions", [[-1, 2], [-2, 3], [-1, -3, -4]], [1, 4], [[-1, 3]], None, None),
        ("quad with its own lemmas", quad, [], solve(quad)["kept"], None, None),
        ("limit with a carry", php4, [], php4_part, None, None),      # (conflict_limit 2 in the tests)
        ("room equal to the carry: SAT", [[1, 2]], [], [[1, 2, 3]], 4, None),
        ("room equal to the carry: FULL", php4, [], php4_part, R.region_words(php4_part), None),
        ("room one short of the closing record", php3, [], php3_kept, R.region_words(php3_kept), None),
        ("literal beyond inst_nvars with a carry", [[1, 4]], [], [[1]], None, 3),
        ("bogus: carried literal beyond inst_nvars", [[1, 2]], [], [[1], [4]], None, 3),
        ("bogus: carry larger than the room", [[1, 2]], [], [[1, 2], [2]], 4, None),
        ("bogus unit makes a satisfiable formula UNSAT", [[1, 2], [-1, 2]], [], [[-2]], None, None),
    ]
    out += [(f"carried lemma of {k}",) + wide_carry_row(k) + (None, None) for k in (1, 63, 64, 65)]
    rng = random.Random(CHAIN_SEED + 1)
    for i in range(24):     # chains as rows: query j carries query j-1's kept list
        kept = []
        for j, (f, a) in enumerate(random_chain(rng, 12)):
            out.append((f"chain {i} query {j}", f, a, kept, None, None))
            kept = solve(f, a, 0, kept)["kept"]
    return out


LIMITS = {"limit with a carry": 2}      # conflict_limit of a row (0 elsewhere)
