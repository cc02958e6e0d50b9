"""The rows at which the certificate kernels (csrc/check.hip, refute.hip,
trim.hip, witness.hip) meet the solvers' structural path rows, and the plain
references the certificates are held to; shared by tests/test_cert_rows.py
(CPU: the selection is what it claims) and tests/test_cert_paths_gpu.py (GPU:
every verdict at these rows is certified).

The rows are those of tests/dp_paths.py and tests/res_paths.py that run to a
verdict, and the formula lists of the two batched solvers' tests.  The path
tests compare a kernel's record with the oracle's, clause by clause; a
certificate does not care where a record came from: a core must be
unsatisfiable, a rebuilt model must satisfy every clause.  What is plain here
(satisfies, Rup, plain_unsat, chain_model) is independent of the certifier
kernels and of the oracle.  unsat_by_oracle enumerates up to 20 variables and
asks the CPU oracle beyond; since the oracle's CDCL never answers False, that is
its Davis-Putnam elimination alone -- no certifier, but for a whole path row the
very run that gave the verdict, so the rows' own unsatisfiability is shown by
plain_unsat and by the plain forward check of the record (tests/test_cert_rows.py),
and unsat_by_oracle adds to them only on cores, which are other clause sets."""
import functools
import os

import dp_batch_rows
import dp_paths
import oracle
import paths_rows
import res_batch_rows
import res_paths

TRIM_MAX_VARS, REFUTE_MAX_VARS, WITNESS_MAX_VARS = 16383, 32767, 524287
SHORT_MAX = 8            # RF_SHORT_MAX, TR_SHORT_MAX, WT_SHORT_MAX: the longest clause of the lane-per-clause forms
FORWARD_P_MAX = 8384     # chain_129_unsat's record: every False row up to it goes through the forward check whole
CDCL_MAX_ITER = 2000     # unsat_by_oracle: past it the oracle's Davis-Putnam decides (the reference's CDCL, which the
                         # oracle restates, learns without end on an unsatisfiable formula: every False row gets here)
BRUTE_MAX_VARS = 20      # unsat_by_oracle: up to here plain enumeration decides

CHAIN_SIZES = (64, 65, 128, 129, 192, 193, 256, 257, 300)

# name -> (verdict, record clauses P, largest id, longest clause of formula and record) of the
# Davis-Putnam rows that run to a verdict, as the oracle runs them (a chain of n: the lists after
# the steps hold n - 1, n - 2, .. clauses, and one more each while [-xn] waits for its variable)
DP_TABLE = {}
for _n in CHAIN_SIZES:
    DP_TABLE["chain_%d_sat" % _n] = (1, _n * (_n - 1) // 2, None, 2)
    DP_TABLE["chain_%d_unsat" % _n] = (0, _n * (_n - 1) // 2 + _n - 1, None, 2)
DP_TABLE.update({"disjoint_70": (1, 7982, None, None), "disjoint_130": (1, 29288, None, None),
                 "disjoint_200": (1, 70310, None, None), "disjoint_260": (1, 121767, None, None),
                 "many_20": (0, 724, 20, 6), "php65": (0, 26693, 30, 8)})
DP_MAX_ID = {"chain": (2368, 11100), "disjoint": (2590, 9620)}     # smallest and largest of the rows' largest ids
DISJOINT_LONGEST = (5, 6)

# name -> (verdict, record clauses P) of the resolution rows that reach a verdict
RES_TABLE = {"stage_one_stripe": (1, 600), "stage_present": (1, 600), "abuf": (1, 2560), "pairbuf": (1, 2600),
             "pairbuf_wide": (1, 2600), "chain30": (1, 435), "chain40": (1, 780), "keys_even": (1, 19200)}

# resolution rows whose verdict is False while the formula is satisfiable (the reference resolves
# on tautological premises): asserted by tests/test_cert_rows.py
UNSOUND_FALSE = []


# ---------------------------------------------------------------- the plain references

def satisfies(formula, model):
    """Whether `model` (signed literals, one per variable) satisfies every clause: a dict lookup per literal."""
    value = {abs(l): l > 0 for l in model}
    return all(any(value.get(abs(l)) == (l > 0) for l in c) for c in formula)


def falsified(formula, model):
    """Indices of the clauses `model` does not satisfy."""
    value = {abs(l): l > 0 for l in model}
    return [i for i, c in enumerate(formula) if not any(value.get(abs(l)) == (l > 0) for l in c)]


def drop_clause(formula, i):
    return [c for k, c in enumerate(formula) if k != i]


def variables(formula):
    return sorted({abs(l) for c in formula for l in c})


def brute_unsat(clauses):
    """Whether no assignment of the (at most BRUTE_MAX_VARS) variables satisfies `clauses`: all of
    them at once, one bit of a numpy word per variable."""
    import numpy as np
    ids = variables(clauses)
    assert len(ids) <= BRUTE_MAX_VARS
    bit = {v: k for k, v in enumerate(ids)}
    a = np.arange(1 << len(ids), dtype=np.uint32)
    alive = np.ones(a.shape, dtype=bool)
    for c in clauses:
        sat = np.zeros(a.shape, dtype=bool)
        for l in c:
            sat |= ((a >> np.uint32(bit[abs(l)])) & np.uint32(1)) == (1 if l > 0 else 0)
        alive &= sat
    return not alive.any()


def unsat_by_oracle(clauses):
    """Whether `clauses` are unsatisfiable.  Up to BRUTE_MAX_VARS variables by enumeration (the
    batched rows hold repeated literals, tautologies and empty clauses, on which the reference's
    solvers, and so the oracle, are not to be trusted).  Beyond that by the CPU oracle: its
    CDCL, whose True counts only with its model checked by satisfies, and where that runs into
    the iteration cap its Davis-Putnam elimination."""
    clauses = [list(c) for c in clauses]
    if any(len(c) == 0 for c in clauses):
        return True
    if len(variables(clauses)) <= BRUTE_MAX_VARS:
        return brute_unsat(clauses)
    r = oracle.cdcl(clauses, max_iter=CDCL_MAX_ITER)
    if r["result"] == 0:
        return True
    if r["result"] == 1:
        given = {abs(l) for l in r["assignment"]}
        if satisfies(clauses, list(r["assignment"]) + [-v for v in variables(clauses) if v not in given]):
            return False
    return oracle.dp(clauses)["result"] == 0


class Rup:
    """Unit propagation in plain Python over a growing list of premises (tests/refute_rows.py's
    rule for clauses without bad literals): occurrence lists and a queue in place of the naive
    rounds, so that a proof of thousands of lemmas is checked in seconds."""

    def __init__(self, premises=()):
        self.clauses, self.occurs, self.short = [], {}, []
        for c in premises:
            self.add(c)

    def add(self, clause):
        c = set(clause)
        k = len(self.clauses)
        self.clauses.append(c)
        if any(-l in c for l in c):
            return                        # a tautological premise never forces anything
        if len(c) <= 1:
            self.short.append(k)
        for l in c:
            self.occurs.setdefault(l, []).append(k)

    def conflict(self, lemma):
        """Whether assigning every literal of `lemma` false and propagating to a fixpoint
        reaches a conflict."""
        if any(-l in lemma for l in lemma):
            return True
        value, queue = {}, []

        def assign(l):
            if abs(l) not in value:
                value[abs(l)] = l > 0
                queue.append(l)
                return True
            return value[abs(l)] == (l > 0)

        def visit(k):
            free = None
            for l in self.clauses[k]:
                v = value.get(abs(l))
                if v is None:
                    if free is not None:
                        return True
                    free = l
                elif v == (l > 0):
                    return True
            return free is not None and assign(free)

        for l in lemma:
            assign(-l)
        if not all(visit(k) for k in self.short):
            return True
        at = 0
        while at < len(queue):
            l = queue[at]
            at += 1
            for k in self.occurs.get(-l, ()):
                if not visit(k):
                    return True
        return False


def rup_conflict(premises, lemma):
    return Rup(premises).conflict(lemma)


def rup_proof(formula, proof):
    """The forward check in plain Python: every lemma up to the first empty one follows by unit
    propagation from the formula and the lemmas before it, and an empty lemma is reached."""
    rup = Rup(formula)
    for lemma in proof:
        if not rup.conflict(lemma):
            return False
        if not lemma:
            return True
        rup.add(lemma)
    return False


def plain_unsat(clauses, node_limit=200000):
    """Whether `clauses` are unsatisfiable, decided by a plain DPLL search in Python (unit
    propagation by simplification, then a branch on the first literal of a shortest clause):
    independent of the oracle and of every kernel.  A chain falls to propagation alone; the
    pigeons of php65 take a few thousand branches.  Raises past `node_limit` branches."""
    nodes = [0]

    def simplify(cs, l):
        out = []
        for c in cs:
            if l in c:
                continue
            out.append(c - {-l} if -l in c else c)
        return out

    def satisfiable(cs):
        while True:
            if not cs:
                return True
            if any(not c for c in cs):
                return False
            unit = next((c for c in cs if len(c) == 1), None)
            if unit is None:
                break
            cs = simplify(cs, next(iter(unit)))
        nodes[0] += 1
        if nodes[0] > node_limit:
            raise RuntimeError("plain_unsat: node limit")
        l = min(min(cs, key=len))
        return satisfiable(simplify(cs, l)) or satisfiable(simplify(cs, -l))

    cs = [frozenset(c) for c in clauses]
    return not satisfiable([c for c in cs if not any(-l in c for l in c)])


# ---------------------------------------------------------------- Davis-Putnam rows

def dp_rows():
    """The rows of dp_paths.ROWS that run to their verdict."""
    return [n for n, (_, step_limit, _) in dp_paths.ROWS.items() if step_limit == 0]


def res_rows():
    """The rows of tests/res_paths.py whose oracle run reaches a verdict with neither max_passes
    nor clause_limit: those tests/golden/paths_res.json marks complete, and keys_even, which
    the oracle saturates in its second pass (the reference was not given the time).  The width
    rows and php43x3 grow without end in sight on both sides."""
    fx = paths_rows.load(os.path.join(paths_rows.HERE, "golden"), "res")["rows"]
    names = [n for n in paths_rows.res_rows() if paths_rows.res_base(n) == n and fx[n]["complete"]]
    return names + ["keys_even"]


@functools.lru_cache(maxsize=None)
def formula(kind, name):
    if kind == "dp":
        return dp_paths.row_formula(name)
    f = res_paths.row(name)[0]
    fx = paths_rows.load(os.path.join(paths_rows.HERE, "golden"), "res")["rows"][name]
    assert paths_rows.formula_sha(f) == fx["formula_sha"], name
    return f


@functools.lru_cache(maxsize=None)
def oracle_run(kind, name):
    """The oracle's recorded run of a row, once per process."""
    if kind == "dp":
        return dp_paths.row_oracle(name)
    return oracle.resolution(formula(kind, name), record=True, rec_cap=1 << 23)


def record(run):
    """A recorded run's clauses, flat, in order (satmi.witness.record_of's order)."""
    return [list(c) for group in run["clauses"] for c in group]


def rows():
    """[(kind, name)] of every path row with a verdict."""
    return [("dp", n) for n in dp_rows()] + [("res", n) for n in res_rows()]


def verdict(kind, name):
    return oracle_run(kind, name)["result"]


def table(kind, name):
    """(verdict, record clauses P) a row is listed with: what tests parametrise from, the
    oracle's runs staying inside the tests (tests/test_cert_rows.py holds the tables to them)."""
    return (DP_TABLE if kind == "dp" else RES_TABLE)[name][:2]


def table_rows(verdict_):
    """[(kind, name)] of the rows listed with this verdict, from the tables alone."""
    return [("dp", n) for n, t in DP_TABLE.items() if t[0] == verdict_] + \
        [("res", n) for n, t in RES_TABLE.items() if t[0] == verdict_]


def longest(kind, name):
    return max(len(c) for c in formula(kind, name) + record(oracle_run(kind, name)))


def forward_rows():
    """The False rows whose whole record goes through the forward check: P <= FORWARD_P_MAX, and
    php65, the one row at the clause forms' threshold."""
    return [(k, n) for k, n in rows() if verdict(k, n) == 0 and
            (len(record(oracle_run(k, n))) <= FORWARD_P_MAX or n == "php65")]


# ---------------------------------------------------------------- chains

def chain_parts(name):
    """(n, x) of a chain row: x[i] the id of the chain's i-th variable, as dp_paths.chain draws it."""
    import random
    n = int(name.split("_")[1])
    seed = 301 if name == "chain_300_unsat" else n
    rng = random.Random(seed)
    img = list(range(1, n + 1))
    rng.shuffle(img)
    return n, [0] + [37 * v for v in img]


def chain_positions(name):
    """Indices, in the shuffled formula of chain_*_unsat, of the unit [x1], of [-xn] and of the
    link [-xk, x(k+1)] with k = n // 2."""
    n, x = chain_parts(name)
    f = dp_paths.row_formula(name)
    k = n // 2
    return f.index([x[1]]), f.index([-x[n]]), f.index([-x[k], x[k + 1]])


def chain_model(name, which):
    """A model of the chain with one clause dropped (which = 0: [x1], 1: [-xn], 2: the link k ->
    k + 1): all False; all True; True up to xk and False behind it."""
    n, x = chain_parts(name)
    k = n // 2
    sign = {0: lambda i: -1, 1: lambda i: 1, 2: lambda i: 1 if i <= k else -1}[which]
    return sorted((sign(i) * x[i] for i in range(1, n + 1)), key=abs)


def chain_unsat_rows():
    return [n for n in dp_rows() if n.startswith("chain_") and n.endswith("_unsat")]


# ---------------------------------------------------------------- batched rows

def batch_rows():
    """name -> (kind, formulas, clause capacity set through debug_batch or 0): the lists of
    tests/dp_batch_rows.py and tests/res_batch_rows.py as their GPU tests hand them to
    eliminate_batch / resolve_batch.  dp_capacity runs at SMALL_CAP, where the batched kernel
    hands the longer lists back to the single call; dp_edge and dp_wave hold one such row each
    at any capacity."""
    D, R = dp_batch_rows, res_batch_rows
    return {"dp_edge": ("dp", D.EDGE, 0), "dp_mix": ("dp", D.mix(), 0), "dp_sparse_mix": ("dp", D.sparse_mix(), 0),
            "dp_capacity": ("dp", D.capacity_rows(), D.SMALL_CAP),
            "dp_wave": ("dp", [D.WAVE_ROWS[k] for k in D.WAVE_ROWS] + [D.D32], 0),
            "res_edge": ("res", R.EDGE, 0), "res_mix": ("res", R.mix(), 0)}


@functools.lru_cache(maxsize=None)
def batch_verdicts(name):
    kind, fs, _ = batch_rows()[name]
    solve = oracle.dp if kind == "dp" else oracle.resolution
    return tuple(solve(f)["result"] for f in fs)


# list -> (True answers, False answers) of the oracle; no list lacks either (tests/test_cert_rows.py)
BATCH_COUNTS = {"dp_edge": (7, 3), "dp_mix": (88, 112), "dp_sparse_mix": (15, 25), "dp_capacity": (15, 17),
                "dp_wave": (5, 7), "res_edge": (5, 3), "res_mix": (133, 67)}
# list -> (the True answers whose formula is unsatisfiable, the False answers whose formula is
# satisfiable), by batch_unsound: the reference answers True whenever a formula holds the empty
# clause beside others, and its resolution resolves [v, -v, ..] on v
BATCH_UNSOUND = {"dp_edge": ((1, 6), ()), "res_edge": ((1, 6), (7,)), "res_mix": ((), (44, 176, 187))}


@functools.lru_cache(maxsize=None)
def batch_unsound(name):
    """(indices of the True answers whose formula is unsatisfiable, of the False answers whose
    formula is satisfiable): the reference answers True for a formula that holds the empty
    clause and resolves on tautological premises."""
    _, fs, _ = batch_rows()[name]
    v = batch_verdicts(name)
    true = tuple(b for b, f in enumerate(fs) if v[b] == 1 and unsat_by_oracle(f))
    false = tuple(b for b, f in enumerate(fs) if v[b] == 0 and not unsat_by_oracle(f))
    return true, false
