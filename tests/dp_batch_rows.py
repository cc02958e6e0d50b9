"""Formulas that drive the batched Davis-Putnam kernel (csrc/dp_batch.hip)
through each of its paths, and the proofs that they do, shared by
tests/test_dp_batch.py (CPU: every row has the sizes, the variable order and
the collision step it claims, derived from the oracle's record) and
tests/test_dp_batch_gpu.py (GPU: every row exact against the oracle).

What decides a path in csrc/dp_batch.hip, in the kernel's terms:

  d       distinct variables: at most 31 (one key P | N << 32), else UNFIT;
  live    the ids of the variables a step still sees: their home slots in the
          table of a fresh set (satmi.dp.order_free_pop) must be distinct,
          else UNFIT at that step; the popped id is the lowest home's;
  ncl, np, nn, kept   list, pos, neg and kept-resolvent counts of a step: a wave
          step is 64 lanes, compaction prefixes cross it at 63 / 64 / 65;
  pairs   np * nn, streamed in chunks of CHUNK pairs;
  cap     the clause capacity: a completed list longer than it is UNFIT; a
          step that ends the elimination completes none.
"""
import functools
import itertools
import random

import oracle
from satmi.dp import order_free_pop

CHUNK = 1024        # DPB_CHUNK
MAXVARS = 31        # DPB_MAXVARS
CAP_MAX = 1920      # the largest tier's clause capacity


def lit_order(clause):
    """The batch record's literal order: ascending variable id, +v before -v."""
    return sorted(set(clause), key=lambda l: (abs(l), l < 0))


def variables(clauses):
    return sorted({abs(l) for c in clauses for l in c})


def completed(o):
    """Steps of an elimination result o (the oracle's or eliminate_batch's
    dict with a record) that completed a clause list.  The step that ends an
    elimination with 0 / -1 completes none; the oracle's record shows it as an
    empty list, which no completed step under those verdicts can leave (an
    empty list ends the loop with True before any limit is looked at)."""
    n = min(o["steps"], len(o["clauses"]))
    return n if n == 0 or o["result"] == 1 or len(o["clauses"][n - 1]) > 0 else n - 1


def profile(f, step_limit=0, clause_limit=0):
    """The oracle's elimination of f, step by step, from its record: per step the
    live ids, whether their homes collide, the popped id the slot rule gives,
    and the list / pos / neg / rest / pair / kept counts."""
    o = oracle.dp(f, step_limit=step_limit, clause_limit=clause_limit, record=True)
    lists = [[list(c) for c in f]] + o["clauses"][:completed(o)]
    steps = []
    for k, var in enumerate(o["vars"]):
        cur = [set(c) for c in lists[k]]
        live = variables(cur)
        np_ = sum(var in c for c in cur)
        nn = sum(-var in c for c in cur)
        nr = sum(var not in c and -var not in c for c in cur)
        row = {"var": var, "live": live, "rule": order_free_pop(live), "ncl": len(cur), "np": np_, "nn": nn,
               "nr": nr, "pairs": np_ * nn, "completed": k + 1 < len(lists)}
        if row["completed"]:
            row["next"] = len(lists[k + 1])
            row["kept"] = row["next"] - nr
        steps.append(row)
    collide = next((k for k, s in enumerate(steps) if s["rule"] is None), None)
    return {"oracle": o, "steps": steps, "collide_step": collide, "d": len(variables(f)),
            "max_list": max(len(l) for l in lists), "lists": lists}


def fits(p, cap=CAP_MAX):
    """Does the batched kernel take the formula of profile p at capacity cap?"""
    return p["d"] <= MAXVARS and p["collide_step"] is None and p["max_list"] <= cap


def model(f, step_limit=0, clause_limit=0):
    """REF.py:98-130 restated on frozensets with the slot rule in place of the
    set images -- what the kernel computes, on the host.  Returns the oracle's
    dict shape plus per-step events: for every step (nr, non-tautological
    resolvents, pair index of the first empty resolvent or None, resolvents
    before it); "result" is None where the rule gives no variable."""
    clauses = [frozenset(c) for c in f]
    out = {"result": 1, "vars": [], "steps": 0, "clauses": [], "events": []}
    while True:
        live = variables(clauses)
        if not live:
            return out
        if step_limit > 0 and out["steps"] >= step_limit:
            out["result"] = -1
            return out
        var = order_free_pop(live)
        if var is None:
            out["result"] = None
            return out
        out["vars"].append(var)
        out["steps"] += 1
        pos = [c for c in clauses if var in c]
        neg = [c for c in clauses if -var in c]
        nxt = [c for c in clauses if var not in c and -var not in c]
        nr, cnt, empty_at, before = len(nxt), 0, None, 0
        verdict = None
        new = []
        for p, (a, b) in enumerate(itertools.product(pos, neg)):
            r = (a - {var}) | (b - {-var})
            if any(-l in r for l in r):
                continue
            if not r:
                if empty_at is None:
                    empty_at, before = p, cnt
                if verdict is None:
                    verdict = 0
                continue
            cnt += 1
            new.append(r)
            if verdict is None and clause_limit > 0 and nr + cnt > clause_limit:
                verdict = -1
        out["events"].append((nr, cnt, empty_at, before))
        if verdict is not None:
            out["result"] = verdict
            return out
        for r in new:
            if not any(e <= r for e in nxt):
                nxt.append(r)
        clauses = nxt
        out["clauses"].append([lit_order(c) for c in clauses])


# ---------------------------------------------------------------- the rows
# (the last but one: {5, 13} share home 5 of 8 slots, so by the slot rule it is the
# one row of these that the kernel hands back; {5, 14} beside it does not collide)
EDGE = [[], [[]], [[1]], [[1], [-1]], [[1, -1]], [[1, 1], [-1]], [[1, 2], [], [-1]], [[1, -1], [1], [-1]],
        [[5], [-5, 13]], [[5], [-5, 14]]]

SLOT = [[1, 2, 3], [-1, 4, 5], [-2, 9, 3], [4, -5, 9], [-3, -9, 5], [1, -4, 9], [2, 5, -9]]
SLOT37 = [[37 * l for l in c] for c in SLOT]
COLLIDE0 = [[1, 9], [-1, -9]]                                   # {1, 9}: both at home 1 of 8 slots
COLLIDE1 = [[2, 3], [-2, 4], [9, 17], [-9, 3], [4, -17]]        # 5 ids, 32 slots: distinct; then {3, 4, 9, 17} in 8


@functools.lru_cache(maxsize=None)
def mix():
    """200 formulas over ids <= 8 (no live set of them can collide in 8 or 32
    slots): n in 2..8, m in 1..30, clauses of 1..4 literals, every 7th with a
    duplicate clause, every 11th with a tautological clause."""
    rng = random.Random(29)
    fs = []
    for it in range(200):
        n = rng.randint(2, 8)
        m = rng.randint(1, 30)
        f = [[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), rng.randint(1, min(4, n)))]
             for _ in range(m)]
        if it % 7 == 0:
            f.append(list(f[0]))
        if it % 11 == 0:
            f.append([1, -1, 2])
        fs.append(f)
    return fs


def sparse_mix():
    """The first 40 formulas of mix() with v -> v + 64: every id is above 63, so
    the host encodes them on its sorted path (csrc/batch_keys.h), and the live
    ids 65 .. 72 still sit at distinct homes in 8 and in 32 slots."""
    return [[[l + 64 if l > 0 else l - 64 for l in c] for c in f] for f in mix()[:40]]


def _triples(k, seed):
    """k distinct 3-literal clauses over the variables 2 .. 9, no two on the same
    literals: none is a subset of another."""
    rng = random.Random(seed)
    all3 = [[v if s >> i & 1 else -v for i, v in enumerate(vs)]
            for vs in itertools.combinations(range(2, 10), 3) for s in range(8)]
    return rng.sample(all3, k)


def fan(k, sign, seed=1):
    """k clauses [sign * 1, a, b, c] and the unit [-sign * 1]: variable 1 goes
    first (ids 1 .. 9 sit at their own homes in 32 slots), its step has a pos
    (sign = 1) or neg (sign = -1) list of k, k pairs, and keeps k resolvents;
    the list has k + 1 clauses before it and k after."""
    return [[sign] + t for t in _triples(k, seed)] + [[-sign]]


def grid_pairs(np_, nn, seed=2):
    """np_ clauses with 1 and nn with -1 over the variables 2 .. 9: np_ * nn pairs in step 0."""
    t = _triples(np_ + nn, seed)
    return [[1] + c for c in t[:np_]] + [[-1] + c for c in t[np_:]]


def chain(d):
    """[i, -(i + 1)] over the ids 1 .. d: d variables, no collision for d <= 31."""
    return [[i, -(i + 1)] for i in range(1, d)]


WAVE_ROWS = {
    "pos63": fan(63, 1), "pos64": fan(64, 1), "pos65": fan(65, 1),
    "neg63": fan(63, -1), "neg64": fan(64, -1), "neg65": fan(65, -1),
    "pairs1023": grid_pairs(33, 31), "pairs1024": grid_pairs(32, 32), "pairs1025": grid_pairs(25, 41),
    "pairs2500": grid_pairs(50, 50),
    "d31": chain(31),
}
D32 = chain(32)

SMALL_CAP = 66      # the capacity test's clause capacity: pos65 is a list of exactly 66


def capacity_rows():
    """Rows for the capacity knob at SMALL_CAP: lists over it on input
    (pairs2500, fans of 70 and 80), in a later step (the pairs rows of 64 .. 66 input
    clauses), never (the mix), and one of exactly SMALL_CAP clauses (pos65: 66, then 65, ...)."""
    return mix()[:24] + [WAVE_ROWS[k] for k in ("pairs1023", "pairs1024", "pairs1025", "pairs2500", "pos65", "neg63")] + \
        [fan(70, 1, seed=3), fan(80, -1, seed=4)]


def limit_rows(fs):
    """From fs: (formula, clause_limit that trips before the empty resolvent of
    the step that has one, clause_limit that trips only after it) -- a step with
    an empty resolvent at pair E preceded by c >= 1 non-tautological resolvents,
    and no earlier step whose rest + resolvents reach the first limit."""
    for f in fs:
        ev = model(f)["events"]
        if not ev or ev[-1][2] is None:
            continue
        nr, _, _, before = ev[-1]
        if before < 1:
            continue
        lo, hi = nr + before - 1, nr + before
        if lo < 1 or any(r + c > lo for r, c, _, _ in ev[:-1]):
            continue
        return f, lo, hi
    return None
