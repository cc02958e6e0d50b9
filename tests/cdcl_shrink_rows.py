"""Minimal failed-assumption cores in plain Python, and the rows of their tests
(tests/test_cdcl_shrink_rows.py holds the rule to brute force and to a plain RUP check;
tests/test_cdcl_shrink_gpu.py holds the shrinking kernel of csrc/cdcl_sound.hip to the rule).

The rule is include/satmi.h's (satmi_cdcl_shrink_batch_device): a chain of cdcl_carry_rows.solve
calls on one formula, each carrying the kept lemmas of the one before.  Query 0 runs under the
assumptions as given; when it ends ASSUMED, W is its core and one trial after another runs
under W less W[p]: a trial that ends ASSUMED refines W to its core (in W's order), one that
ends SAT proves W[p] necessary, one that ends LIMIT keeps it unproven.  Nothing here searches:
this file composes the carrying rule and is no second solver."""
import random

import cdcl_assume_rows as A
import cdcl_carry_rows as C
import cdcl_sound_rows as R

UNSAT, SAT, LIMIT, FULL, TOO_LARGE, ASSUMED = range(6)
COUNTERS = R.COUNTERS
MAX_LEVEL = COUNTERS.index("max_level")
SHRINK = ("queries", "sat_trials", "assumed_trials", "limit_trials", "first_core", "reserved")
TRUNCATED = C.TRUNCATED


def solve(formula, assumptions=(), conflict_limit=0, carry=(), room=None, nvars=None, **rule):
    """cdcl_carry_rows.solve's dict for the whole chain ("hits" left out): the counters summed
    over the queries (max_level their maximum), "lemmas" the region's records at the end,
    "core" the final W, and with it "shrink" (the six words of SHRINK), "first" (query 0's
    result), "trials" (the (dropped literal, status) pairs in order) and "queries" (every
    query's own result, query 0's first).  `rule` = cdcl_carry_rows.solve's keywords for
    another rule, in every query."""
    clauses = [list(c) for c in formula]
    top = max([abs(l) for c in clauses + [list(c) for c in carry] for l in c] + [abs(a) for a in assumptions] + [0])
    nv = top if nvars is None else nvars
    first = C.solve(clauses, assumptions, conflict_limit, carry, room, nv, **rule)
    out = {k: first[k] for k in ("status", "model", "lemmas", "core", "kept", "records", "words", "flags")}
    out["counters"] = list(first["counters"])
    out["first"], out["trials"], out["queries"] = first, [], [first]
    n = dict.fromkeys(SHRINK, 0)
    n["queries"] = 1
    out["shrink"] = [n[k] for k in SHRINK]
    if first["status"] != ASSUMED:
        return out
    W, p, last = list(first["core"]), 0, first
    n["first_core"] = len(W)
    while p < len(W):
        trial = W[:p] + W[p + 1:]
        last = C.solve(clauses, trial, conflict_limit, last["kept"], room, nv, **rule)
        out["queries"].append(last)
        n["queries"] += 1
        out["trials"].append((W[p], last["status"]))
        for i, x in enumerate(last["counters"]):
            out["counters"][i] = max(out["counters"][i], x) if i == MAX_LEVEL else out["counters"][i] + x
        st = last["status"]
        if st == ASSUMED:
            assert all(x in last["core"] for x in W[:p]), "a necessary literal left the core"
            assert set(last["core"]) <= set(trial)
            W = [x for x in trial if x in last["core"]]
            n["assumed_trials"] += 1
        elif st == SAT:
            p += 1
            n["sat_trials"] += 1
        elif st == LIMIT:
            p += 1
            n["limit_trials"] += 1
        else:       # UNSAT: the formula alone is refuted; FULL: the region is too small
            assert st in (UNSAT, FULL), st
            out.update(status=st, core=[] if st == UNSAT else None, lemmas=last["lemmas"], kept=last["kept"],
                       records=last["records"], words=last["words"], flags=last["flags"],
                       shrink=[n[k] for k in SHRINK])
            return out
    # the end: ASSUMED with core W, the region closed by one empty record
    kept = last["kept"]
    words = R.region_words(kept) + 1
    fits = room is None or words <= room
    out.update(status=ASSUMED if fits else FULL, core=W if fits else None, kept=kept,
               lemmas=kept + [[]] if fits else list(kept), records=len(kept) + 1, words=words,
               flags=0 if fits else TRUNCATED, shrink=[n[k] for k in SHRINK])
    return out


def host_chain(query, formula, assumptions=(), conflict_limit=0, carry=()):
    """The same chain over any carrying entry point: query(formula, assumptions, conflict_limit,
    carry) -> a dict with "status", "core", "kept" and "counters" (a name -> count dict).
    Returns (status, core, kept, summed counters as a list)."""
    r = query(formula, list(assumptions), conflict_limit, [list(c) for c in carry])
    total = [r["counters"][k] for k in COUNTERS]
    if r["status"] != ASSUMED:
        return r["status"], r["core"], r["kept"], total
    W, p = list(r["core"]), 0
    while p < len(W):
        trial = W[:p] + W[p + 1:]
        r = query(formula, trial, conflict_limit, r["kept"])
        for i, k in enumerate(COUNTERS):
            total[i] = max(total[i], r["counters"][k]) if i == MAX_LEVEL else total[i] + r["counters"][k]
        if r["status"] == ASSUMED:
            W = [x for x in trial if x in r["core"]]
        elif r["status"] in (SAT, LIMIT):
            p += 1
        else:
            return r["status"], [] if r["status"] == UNSAT else None, r["kept"], total
    return ASSUMED, W, r["kept"], total


# ---- the rows
HAND = ([[-1, -2, 4], [-2, 4], [-3, -4]], [1, 2, 3])


def php_groups_row(idle=0):
    """PHP(3), every clause carrying one of six negated selectors in turn, under the six (with
    `idle` selectors of no clause in front): every group is needed."""
    f, _ = A.php_selector_row()
    return f, list(range(20, 20 + idle)) + A.SELECTORS


def unsat_trial_row():
    """PHP(3) beside [-s, x], [-s, -x] under [s]: s is refuted, and without it PHP(3) remains."""
    s, x = 13, 14
    return R.php(3) + [[-s, x], [-s, -x]], [s]


def wide_row(long_clause):
    """70 selectors 1 .. 70.  1 .. 68 together imply x, by one clause of 69 literals or by a chain
    of 3-literal clauses; x refutes 70; and 2 and 68 alone imply x by a route that is one round
    slower.  Query 0 blames 70 and all of 1 .. 68; the minimal core is 70, 68, 2, the first two
    and the last but one of W."""
    k, c, w = 68, 70, 70 + 68 + 1
    x = c + k
    if long_clause:
        f = [[-v for v in range(1, k + 1)] + [x]]
    else:
        f = [[-1, c + 1]] + [[-(c + i - 1), -i, c + i] for i in range(2, k + 1)]
    f += [[-2, -k, w], [-w, x], [-x, -70]]
    return f, list(range(1, 71))


def random_row(rng):
    n = rng.randint(6, 10)
    f = [[rng.choice((1, -1)) * v for v in rng.sample(range(1, n + 1), 3)] for _ in range(int(3.6 * n))]
    return f, [rng.choice((1, -1)) * v for v in rng.sample(range(1, n + 1), rng.randint(3, 6))]


RANDOM_SEED, RANDOM_COUNT = 0x5812, 320
LIMITS = {}         # conflict_limit of a row (0 elsewhere)


def _find(what, seed, accept, most=4000):
    rng = random.Random(seed)
    for _ in range(most):
        row = accept(*random_row(rng))
        if row:
            return row
    raise AssertionError("no seeded row: " + what)


def _limit_row():
    """A random row and a conflict_limit at which query 0 ends ASSUMED and a trial ends LIMIT."""
    def accept(f, a):
        for limit in (1, 2, 3):
            r = solve(f, a, limit)
            if r["first"]["status"] == ASSUMED and r["shrink"][3] >= 1 and r["status"] == ASSUMED:
                return f, a, limit
    return _find("a LIMIT trial", RANDOM_SEED + 1, accept)


def _full_trial_row():
    """A random row in a room that holds query 0's region and not a trial's first lemma."""
    def accept(f, a):
        r = solve(f, a)
        room = r["first"]["words"]
        if r["first"]["status"] == ASSUMED and solve(f, a, 0, (), room)["status"] == FULL:
            assert solve(f, a, 0, (), room)["shrink"][0] > 1
            return f, a, room
    return _find("a FULL trial", RANDOM_SEED + 2, accept)


def _full_close_row():
    """A random row in a room one word short of the closing record behind the last trial."""
    def accept(f, a):
        r = solve(f, a)
        if r["status"] != ASSUMED or r["trials"][-1][1] != SAT:
            return None
        s = solve(f, a, 0, (), r["words"] - 1)
        if s["status"] == FULL and s["shrink"] == r["shrink"] and s["kept"] == r["kept"]:
            return f, a, r["words"] - 1
    return _find("a closing record that does not fit", RANDOM_SEED + 3, accept)


def _carry_row():
    """A random row whose query 0 is ASSUMED, carrying the lemmas of a search on the same formula
    under other assumptions, which it shrinks with."""
    def accept(f, a):
        kept = C.solve(f, [-x for x in a[:2]])["kept"]
        r = solve(f, a, 0, kept)
        if kept and r["status"] == ASSUMED and len(r["core"]) < r["shrink"][4]:
            return f, a, kept
    return _find("a carry", RANDOM_SEED + 4, accept)


def rows():
    """(name, formula, assumptions, carry, room, nvars) tuples: every row of the kernel's parity
    test.  What a row is there for is asserted here, on the rule."""
    out = [("hand row",) + HAND + ([], None, None),
           ("php 3 under its six selectors",) + php_groups_row() + ([], None, None),
           ("php 3 with two idle selectors in front",) + php_groups_row(2) + ([], None, None),
           ("unsat trial",) + unsat_trial_row() + ([], None, None),
           ("70 selectors, a chain",) + wide_row(False) + ([], None, None),
           ("70 selectors, a long clause",) + wide_row(True) + ([], None, None),
           ("no assumptions", R.php(3), [], [], None, None),
           ("sat under its assumptions", [[1, 2], [-1, 3]], [1, -2], [], None, None),
           ("contradicting assumptions", [[1, 2]], [3, 3, -3], [], None, None),
           ("literal beyond inst_nvars", [[1, 4]], [1], [], None, 3)]
    r = solve(*HAND)
    assert r["first"]["core"] == [3, 2, 1] and r["core"] == [3, 2] and r["shrink"] == [4, 2, 1, 0, 3, 0]
    for idle in (0, 2):
        r = solve(*php_groups_row(idle))
        assert r["core"] == r["first"]["core"] and sorted(r["core"]) == A.SELECTORS
        assert r["shrink"] == [7, 6, 0, 0, 6, 0]
    r = solve(*unsat_trial_row())
    assert r["first"]["status"] == ASSUMED and r["first"]["core"] == [13]
    assert r["status"] == UNSAT and r["core"] == [] and r["trials"] == [(13, UNSAT)] and r["lemmas"][-1] == []
    assert A.refutes(unsat_trial_row()[0], r["lemmas"])
    for long_clause in (False, True):
        f, a = wide_row(long_clause)
        r = solve(f, a)
        W = r["first"]["core"]
        assert W == [70] + list(range(68, 0, -1)) and r["core"] == [70, 68, 2]
        assert [W.index(x) for x in r["core"]] == [0, 1, 67]        # on both sides of position 64
        assert (max(map(len, f)) > R.SHORT_MAX) == long_clause
    f, a, limit = _limit_row()
    out.append(("limit in a trial", f, a, [], None, None))
    LIMITS["limit in a trial"] = limit
    f, a, room = _full_trial_row()
    out.append(("full in a trial", f, a, [], room, None))
    f, a, room = _full_close_row()
    out.append(("full at the closing record", f, a, [], room, None))
    f, a, kept = _carry_row()
    out.append(("carry in", f, a, kept, None, None))
    rng = random.Random(RANDOM_SEED)
    rand = [(f"random {i}",) + random_row(rng) + ([], None, None) for i in range(RANDOM_COUNT)]
    refuted = [want(r) for r in rand if want(r)["first"]["status"] == ASSUMED]
    shrunk = [w for w in refuted if w["status"] == ASSUMED and len(w["core"]) < w["shrink"][4]]
    assert len(refuted) >= 100 and 3 * len(shrunk) >= len(refuted), (len(shrunk), len(refuted))
    return out + rand


_WANT = {}


def want(row):
    """The rule's result at a row (computed once, shared and never changed)."""
    if row[0] not in _WANT:
        _, f, a, carry, room, nv = row
        _WANT[row[0]] = solve(f, a, LIMITS.get(row[0], 0), carry, room, nv)
    return _WANT[row[0]]
