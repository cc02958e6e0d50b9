"""Small hard "cores" and their renamings, shared by tests/test_oracle_renaming.py
(CPU) and test_dpll_gpu.py::test_scan_kernel_classes_decide_unsat (GPU).

The SOUND search of oracle/sat_oracle.c is equivariant under an injective
renaming of variables (test_oracle_renaming.py): status, counters and the
model (mapped) do not change.  So one small formula whose search exhausts a
tree of 10^3-10^4 nodes, renamed into 1..N, carries that same search into the
clause kernels' layout class of N variables, with the expected results known
from one oracle run on the un-renamed core.

    A  5-SAT at its threshold, n=40, m=845:  5 UNSAT / 11 SAT, 1,375 - 28,416 nodes
    B  4-SAT at its threshold, n=50, m=497 (a 5-slot clause word with a pad
       slot):  5 UNSAT / 3 SAT, 1,526 - 9,214 nodes
    C  3-SAT, n=120, m=511 (m > 448 keeps it out of dpll_fixed_kernel):
       2 UNSAT / 6 SAT, 252 - 12,494 nodes
"""
import functools
import random

import oracle
from satmi import cnf

# core: (instances, n, m, k, seed) of satmi.cnf.uniform_ksat
CORES = {"A": (16, 40, 845, 5, 5040), "B": (8, 50, 497, 4, 4050), "C": (8, 120, 511, 3, 3120)}
CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")


@functools.lru_cache(maxsize=None)
def core_formulas(name):
    count, n, m, k, seed = CORES[name]
    batch = cnf.uniform_ksat(count, n, m, k, seed=seed)
    return tuple(batch.instance(b) for b in range(count))


@functools.lru_cache(maxsize=None)
def core_oracle(name):
    """The oracle's first-model SOUND search of every instance of the core, run once per process."""
    return tuple(oracle.dpll(f, "sound", max_solutions=1, sol_cap=1) for f in core_formulas(name))


def renaming(name, N):
    """img[v] (v = 1..n, img[0] unused): an injective map of the core's variables
    into 1..N that occupies both ends of the range -- some variable lands on N
    itself (the top code of the class) and some on 1.  N == n is the identity."""
    n = CORES[name][1]
    if N == n:
        return list(range(n + 1))
    assert N > n
    rng = random.Random(1000 * N + n)
    img = rng.sample(range(2, N), n - 2) + [1, N]
    rng.shuffle(img)
    return [0] + img


def rename(formula, img):
    return [[img[l] if l > 0 else -img[-l] for l in c] for c in formula]
