"""Rows of the DPLL refutation tests, and the shape of such a proof in plain Python
(tests/test_dpll_proof_rows.py holds the rows to their conditions on the CPU;
tests/test_dpll_refute_gpu.py holds the logging kernels to them).

A SOUND-mode search that ends exhausted with no model logs one lemma per closed
subtree: the clause of the negated decision literals on the path to it, at a
conflict and when a frame is popped after its False phase.  The log is the
post-order walk of the decision tree and ends with the empty clause."""
import random

import refute_rows as rr


def is_postorder(proof):
    """Whether the lemma list is the post-order walk of a binary decision tree: every
    lemma is the negation of a decision path D; an internal node D comes right after the
    subtrees of its two children D + [v] (first, True: v > 0) and D + [-v], a leaf (a
    conflict lemma) after none of its extensions; the last lemma is [] and closes the
    whole tree."""
    if not proof or list(proof[-1]) != []:
        return False
    stack = []   # the paths of the closed subtrees not yet under a parent
    for lemma in proof:
        path = [-l for l in lemma]
        if len({abs(l) for l in path}) != len(path) or 0 in path:
            return False
        under = 0
        while under < len(stack) and stack[-1 - under][:len(path)] == path and len(stack[-1 - under]) > len(path):
            under += 1
        if under == 2:
            first, second = stack[-2], stack[-1]
            v = first[-1]
            if not (v > 0 and first == path + [v] and second == path + [-v]):
                return False
            del stack[-2:]
        elif under != 0:
            return False
        stack.append(path)
    return stack == [[]]


def tree_depth(proof):
    return max(len(c) for c in proof)


# ---- mixed random rows: clause lengths 1 .. 4 over 6 .. 14 variables
# Seeds 0 .. MIXED_COUNT - 1; the oracle decides at least MIXED_UNSAT_MIN of them UNSAT, at
# least MIXED_PURE_MIN of those with pure-literal assignments in the search
# (tests/test_dpll_proof_rows.py asserts both).
MIXED_COUNT = 130
MIXED_UNSAT_MIN, MIXED_PURE_MIN = 40, 10
MIXED_LENS = (1,) + (2,) * 6 + (3,) * 14 + (4,) * 19   # unit clauses are rare: most refutations need decisions


def mixed_row(seed):
    """5 .. 9 clauses per variable over the base variables, and up to three pendant
    variables p with one clause [p, a, b] and one [-p, c] (signs random): p turns pure
    where the search makes c true, below the root."""
    rng = random.Random(0xD9110000 + seed)
    n = rng.randint(6, 14)
    k = rng.randint(0, min(3, n - 5))
    base = n - k

    def lit():
        return rng.choice((1, -1)) * rng.randint(1, base)
    f = [[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, base + 1), min(base, rng.choice(MIXED_LENS)))]
         for _ in range(rng.randint(5 * base, 9 * base))]
    for p in range(base + 1, n + 1):
        s = rng.choice((1, -1))
        f.insert(rng.randrange(len(f) + 1), [s * p, lit(), lit()])
        f.insert(rng.randrange(len(f) + 1), [-s * p, lit()])
    return f


def mixed_rows():
    return [mixed_row(s) for s in range(MIXED_COUNT)]


# ---- 3-SAT rows: (n, m, seed, count) -- alpha = 4.26 and 5, searches under ~2,000 nodes
KSAT_ROWS = ((20, 85, 11, 6), (20, 100, 12, 6), (50, 213, 13, 5), (50, 250, 14, 5))
KSAT_NODE_MAX = 2000


def ksat_rows():
    return [f for n, m, seed, count in KSAT_ROWS for f in rr.random_3sat(count, n, m, seed)]


# ---- bench-shape rows: n = 100, m = 426, UNSAT in under 5,000 nodes by the oracle
BENCH_SEED, BENCH_PICKS = 2026, (4, 12, 59)
BENCH_NODE_MAX = 5000


def bench_rows():
    pool = rr.random_3sat(max(BENCH_PICKS, default=-1) + 1, 100, 426, BENCH_SEED)
    return [pool[i] for i in BENCH_PICKS]


# ---- hand-built formulas
LONG_LEN = 300   # beyond the LDS form's 255-literal clause word: the Wide form


def long_row():
    """A clause of LONG_LEN literals over an UNSAT core on two of its variables."""
    return [list(range(1, LONG_LEN + 1)), [1, 2], [1, -2], [-1, 2], [-1, -2]]


HAND_ROWS = [
    [[]],
    [[1], [-1]],
    [[1, 1, 2], [1, 1, -2], [-1, -1, 2, 2], [-1, -2, -2]],            # duplicate literals
    [[1, -1], [2, -2, 3], [1, 2], [1, -2], [-1, 2], [-1, -2, 3, -3], [-1, -2]],   # tautologies
    [[1, 2], [1, -2], [-1, 2], [-1, -2]],
    [[1, 2], [-1, 2], [3, -3]],                                        # satisfiable
]


# ---- the deep row: lemmas of more than 64 literals under a small tree
DEEP_CHAIN = 72


def deep_row(k=DEEP_CHAIN):
    """Chain variables 1 .. k, helpers k + 1 .. 2k.  The first clause forbids all chain
    variables true; (i, k + i) and (i, -(k + i)) make chain variable i's False branch close
    in one propagation round.  Every variable occurs in both signs (nothing is pure), the
    chain variables occur three times and come first, so the search decides 1, 2, ..
    k - 1 True, propagates -k into a conflict, and closes every False branch at once:
    2 (k - 1) + 1 tree nodes, lemmas of up to k - 1 literals."""
    return [[-i for i in range(1, k + 1)]] + [c for i in range(1, k + 1) for c in ([i, k + i], [i, -(k + i)])]


def all_rows():
    """(name, formula) of every row, in one fixed order."""
    rows = [(f"mixed{s}", f) for s, f in enumerate(mixed_rows())]
    rows += [(f"ksat{i}", f) for i, f in enumerate(ksat_rows())]
    rows += [(f"bench{i}", f) for i, f in enumerate(bench_rows())]
    rows += [(f"hand{i}", f) for i, f in enumerate(HAND_ROWS)]
    rows += [("long", long_row()), ("deep", deep_row())]
    return rows


def satisfiable(formula, nvars):
    """A model (tuple of signed literals) by truth-table enumeration, or None."""
    import numpy as np
    bits = np.arange(1 << nvars, dtype=np.int64)
    alive = np.ones(bits.shape, dtype=bool)          # the assignments that satisfy every clause so far
    for c in formula:
        sat = np.zeros(bits.shape, dtype=bool)
        for l in c:
            sat |= ((bits >> (abs(l) - 1)) & 1) == (1 if l > 0 else 0)
        alive &= sat
    hits = np.flatnonzero(alive)
    if hits.size == 0:
        return None
    return tuple(v if (int(hits[0]) >> (v - 1)) & 1 else -v for v in range(1, nvars + 1))
