"""Drop-in solver entry points of the reference script, backed by the GPU.

Same names, signatures, argument meaning and return values as
REF.py ("comparatie intre algoritmii de rezolvare a seturilor de clauze.py"):

    generate_large_formula(num_clauses, max_literals_per_clause, num_variables)  REF.py:21-29
    resolution_solver(formula) -> bool                                           REF.py:63-95
    davis_putnam_solver(formula) -> bool                                         REF.py:98-130
    dpll_optimized(formula, assignment=None) -> List[Assignment]                 REF.py:133-214
    cdcl_solve(formula) -> Tuple[bool, Optional[Assignment]]                     REF.py:217-384
    hybrid_solver(formula, threshold=1000) -> List[Assignment]                   REF.py:400-404
    pysat_solver(formula) -> List[Assignment]                                    REF.py:387-397

Beside them, what makes an answer checkable: check_assignment (a model),
check_refutation / trim_refutation (a False of the two saturation solvers, or
the proof dpll_refutation returns with sound DPLL's UNSAT) and
davis_putnam_witness / resolution_witness (a True of theirs, with its model);
cdcl_sound_solve, the library's own clause-learning search, returns a model or a
proof of that kind, and answers for pysat_solver where PySAT is not installed.

The solvers run on the MI355X through libsatmi.so; there is no CPU fallback.
"""
import random
from typing import Dict, List, Optional, Tuple

from . import _capi
from .dpll import dpll_batch
from .incremental import Solver  # noqa: F401  (the query loop: add_clause / solve(assumptions=...))

Literal = int
Clause = List[Literal]
Formula = List[Clause]
Assignment = Dict[int, bool]

# Per-call wall-clock limit (seconds) the comparison driver sets around a solver
# call (REF.py:417-437 runs each solver under a 60 s timeout); 0 = unlimited.
_time_limit = 0.0


class SolverTimeout(Exception):
    pass


def set_time_limit(seconds):
    global _time_limit
    _time_limit = float(seconds or 0.0)


def generate_large_formula(num_clauses: int, max_literals_per_clause: int, num_variables: int) -> Formula:
    """Random CNF, drawing from Python's `random` in the same sequence as REF.py:21-29
    (size ~ randint(1, max), distinct variables by sample(), each negated w.p. 1/2),
    so a seeded `random` produces the reference's formula."""
    pool = range(1, num_variables + 1)
    out: Formula = []
    for _ in range(num_clauses):
        size = random.randint(1, max_literals_per_clause)
        chosen = random.sample(pool, size)
        out.append([v if random.random() < 0.5 else -v for v in chosen])
    return out


def dpll_optimized(formula: Formula, assignment: Optional[Assignment] = None) -> List[Assignment]:
    """Every solution the reference's DPLL returns, in the same order, each dict in
    the same insertion order.  Like REF.py:167 the caller's `assignment` dict is
    extended in place by the root's unit propagation."""
    init = None if assignment is None else [v if b else -v for v, b in assignment.items()]
    cap = 1024
    while True:
        r = dpll_batch([formula], mode="ref", max_solutions=0, sol_cap=cap,
                       inits=None if init is None else [init], time_limit=_time_limit)
        st = int(r.status[0])
        if st == _capi.DPLL_TIMEOUT:
            raise SolverTimeout(f"Timeout after {_time_limit:g} seconds")
        if st != _capi.DPLL_EXHAUSTED:
            raise _capi.SatmiError(f"dpll_optimized: GPU search ended with status {_capi.STATUS_NAMES.get(st, st)}")
        n = r.num_solutions(0)
        if n <= cap:
            break
        cap = n
    if assignment is not None:
        for lit in r.root_assignment(0)[len(init):]:
            assignment[abs(lit)] = lit > 0
    return [{abs(l): l > 0 for l in sol} for sol in r.solutions(0)]


def dpll_solve(formula: Formula):
    """Sound DPLL decision (same propagation / pure-literal / branching rules as
    REF.py's DPLL, decisions applied to the formula).  Returns (sat, model)."""
    r = dpll_batch([formula], mode="sound", max_solutions=1, time_limit=_time_limit)
    st = int(r.status[0])
    if st == _capi.DPLL_TIMEOUT:
        raise SolverTimeout(f"Timeout after {_time_limit:g} seconds")
    if st not in (_capi.DPLL_EXHAUSTED, _capi.DPLL_STOPPED):   # nothing was decided: never an UNSAT verdict
        raise _capi.SatmiError(f"dpll_solve: GPU search ended with status {_capi.STATUS_NAMES.get(st, st)}")
    if r.num_solutions(0) > 0:
        return True, {abs(l): l > 0 for l in r.solutions(0)[0]}
    return False, None


def dpll_refutation_batch(formulas: List[Formula]):
    """dpll_refutation for many formulas in one launch."""
    from .refute import dpll_refutations
    out = []
    for r in dpll_refutations([list(f) for f in formulas], max_solutions=1, time_limit=_time_limit):
        st = r["status"]
        if st == _capi.DPLL_TIMEOUT:
            raise SolverTimeout(f"Timeout after {_time_limit:g} seconds")
        if st not in (_capi.DPLL_EXHAUSTED, _capi.DPLL_STOPPED):   # nothing was decided: never an UNSAT verdict
            raise _capi.SatmiError(f"dpll_refutation: GPU search ended with status {_capi.STATUS_NAMES.get(st, st)}")
        out.append((True, {abs(l): l > 0 for l in r["model"]}) if r["sat"] else (False, r["proof"]))
    return out


def dpll_refutation(formula: Formula):
    """dpll_solve with a certificate either way: (True, model), or (False, proof) where
    `proof` is the search's refutation -- one lemma per closed subtree, the clause of its
    negated decisions, the empty clause last -- and check_refutation(formula, proof) holds."""
    return dpll_refutation_batch([formula])[0]


def check_assignment(formula: Formula, assignment) -> bool:
    """Whether `assignment` (a solver's dict {variable: bool}, or signed literals) is a
    model of `formula`, evaluated on the GPU (satmi/check.py): every clause has a true
    literal, and the assignment is neither contradictory nor malformed."""
    from .check import check_models
    return check_models([formula], [[assignment]])[0][0]["ok"]


def check_refutation(formula: Formula, proof) -> bool:
    """Whether `proof` (an ordered list of lemma clauses that reaches the empty clause, e.g.
    refute.proof_of_resolution of a recorded False answer) refutes `formula`, checked on the
    GPU (satmi/refute.py): every lemma up to the first empty one follows by unit propagation
    from the formula and the lemmas before it."""
    from .refute import check_refutations
    return check_refutations([formula], [proof])[0]["proven"]


def trim_refutation(formula: Formula, proof) -> Optional[Tuple[Formula, List[Clause]]]:
    """The part of a refutation that matters, found on the GPU by the backward check
    (refute.trim_refutations): (core_clauses, trimmed_proof) -- the formula's clauses that
    the refutation uses and the lemmas it needs, in order, the empty clause last -- such that
    check_refutation(core_clauses, trimmed_proof) holds; None when the trim's status is not
    PROVEN (no empty lemma, or a needed lemma does not follow)."""
    from .refute import trim_refutations
    r = trim_refutations([formula], [proof])[0]
    if not r["proven"]:
        return None
    return [list(formula[c]) for c in r["core"]], r["proof"]


def resolution_solver(formula: Formula) -> bool:
    from .resolution import resolution_solve
    return resolution_solve(formula, time_limit=_time_limit)


def resolution_solver_batch(formulas: List[Formula]) -> List[bool]:
    """resolution_solver for many formulas in one launch (small formulas are
    saturated one per workgroup; the others go through resolution_solver's path)."""
    from .resolution import resolution_solve_batch
    return resolution_solve_batch(formulas, time_limit=_time_limit)


def davis_putnam_solver(formula: Formula) -> bool:
    from .dp import davis_putnam_solve
    return davis_putnam_solve(formula, time_limit=_time_limit)


def davis_putnam_solver_batch(formulas: List[Formula]) -> List[bool]:
    """davis_putnam_solver for many formulas in one launch (small formulas are
    eliminated one per workgroup; the others go through davis_putnam_solver's path)."""
    from .dp import davis_putnam_solve_batch
    return davis_putnam_solve_batch(formulas, time_limit=_time_limit)


def _witnesses(formulas: List[Formula], results, stages_of, highest_only, who):
    """(answer, model) per formula from the recorded results of one solver: the True answers
    go through witness.witness_models in one launch."""
    from .witness import record_of, witness_models
    true = [b for b, r in enumerate(results) if r["result"] == 1]
    out: List[Tuple[bool, Optional[Assignment]]] = [(False, None)] * len(results)
    if true:
        fs = [formulas[b] for b in true]
        ws = witness_models(fs, [record_of(results[b]) for b in true],
                            [stages_of(formulas[b], results[b]) for b in true], highest_only)
        for b, w in zip(true, ws):
            if w["status"] != _capi.WITNESS_MODEL:
                raise _capi.SatmiError(f"{who}: the solver answered True for formula {b}, but the assignment "
                                       f"rebuilt from its record falsifies {w['falsified']} of its clauses "
                                       f"(the first: clause {w['first_falsified']}; {w['stuck']} stuck stages)")
            out[b] = (True, {abs(l): l > 0 for l in w["model"]})
    return out


def davis_putnam_witness_batch(formulas: List[Formula]) -> List[Tuple[bool, Optional[Assignment]]]:
    """davis_putnam_witness for many formulas: one batched elimination, one witness launch."""
    from .dp import DavisPutnamLimit, eliminate_batch
    from .witness import stages_of_elimination
    formulas = [list(f) for f in formulas]
    rs = eliminate_batch(formulas, time_limit=_time_limit, record=True)
    for r in rs:
        if r["result"] < 0:
            raise DavisPutnamLimit(f"Davis-Putnam stopped by its limit after {r['steps']} steps")
    return _witnesses(formulas, rs, stages_of_elimination, False, "davis_putnam_witness")


def davis_putnam_witness(formula: Formula) -> Tuple[bool, Optional[Assignment]]:
    """davis_putnam_solver's answer and, for True, a model {variable: bool} of the formula's
    variables, rebuilt on the GPU from the elimination's record (satmi/witness.py) and
    evaluated there against the formula.  Raises SatmiError when the answer is True and the
    rebuilt assignment is no model: the reference answers True for [[1], []]."""
    from .dp import DavisPutnamLimit, eliminate
    from .witness import stages_of_elimination
    r = eliminate(formula, time_limit=_time_limit, record=True)
    if r["result"] < 0:
        raise DavisPutnamLimit(f"Davis-Putnam stopped by its limit after {r['steps']} steps")
    return _witnesses([formula], [r], stages_of_elimination, False, "davis_putnam_witness")[0]


def resolution_witness_batch(formulas: List[Formula]) -> List[Tuple[bool, Optional[Assignment]]]:
    """resolution_witness for many formulas: one batched saturation, one witness launch."""
    from .resolution import ResolutionLimit, resolve_batch
    from .witness import stages_of_resolution
    formulas = [list(f) for f in formulas]
    rs = resolve_batch(formulas, time_limit=_time_limit, record=True)
    for r in rs:
        if r["result"] < 0:
            raise ResolutionLimit(f"resolution stopped by its limit after {r['passes']} passes")
    return _witnesses(formulas, rs, stages_of_resolution, True, "resolution_witness")


def resolution_witness(formula: Formula) -> Tuple[bool, Optional[Assignment]]:
    """resolution_solver's answer and, for True, a model of the formula's variables, rebuilt
    from the saturation's record as davis_putnam_witness does from the elimination's."""
    from .resolution import ResolutionLimit, resolve
    from .witness import stages_of_resolution
    r = resolve(formula, time_limit=_time_limit, record=True)
    if r["result"] < 0:
        raise ResolutionLimit(f"resolution stopped by its limit after {r['passes']} passes")
    return _witnesses([formula], [r], stages_of_resolution, True, "resolution_witness")[0]


def cdcl_sound_solve(formula: Formula, assumptions=None, minimal_core=False):
    """The library's own clause-learning decision procedure (csrc/cdcl_sound.hip):
    (True, model, None) with model {variable: bool} over the formula's variables, or
    (False, None, proof) where `proof` is the learned clauses in learning order, the empty
    clause last, and check_refutation(formula, proof) holds.  Raises SolverTimeout under the
    driver's deadline and SatmiError when the formula is beyond the kernel's layout or its
    learned clauses outgrow their region.
    With `assumptions`, a list of literals (PySAT's solve(assumptions=...) and get_core()),
    the question is whether the formula is satisfiable with all of them true, and the answer
    has a fourth member: (True, model, None, None), the model over the assumptions' variables
    too, or (False, None, proof, core), where `core` lists the assumptions to blame, the
    refuted one first ([]: the formula alone is unsatisfiable), and check_refutation holds for
    the formula plus the core's literals as unit clauses.
    With `minimal_core` (and assumptions) the core is shrunk on the GPU until the formula is
    satisfiable with the core less any one literal (cdcl_sound.cdcl_shrink_batch; a trial query
    that the deadline cuts keeps its literal); `proof` then holds the lemmas of every query."""
    from .cdcl_sound import cdcl_assume_batch, cdcl_shrink_batch, cdcl_sound_batch
    from .refute import proof_of_cdcl
    if assumptions is not None and minimal_core:
        r = cdcl_shrink_batch([list(formula)], [list(assumptions)], time_limit=_time_limit)[0]
    elif assumptions is not None:
        r = cdcl_assume_batch([list(formula)], [list(assumptions)], time_limit=_time_limit)[0]
    else:
        r = cdcl_sound_batch([list(formula)], time_limit=_time_limit)[0]
    st = r["status"]
    if st == _capi.CDCL_SOUND_LIMIT:
        raise SolverTimeout(f"Timeout after {_time_limit:g} seconds")
    if r["sat"] is None:   # nothing was decided: never an UNSAT verdict
        raise _capi.SatmiError("cdcl_sound_solve: GPU search ended with status "
                               f"{_capi.CDCL_SOUND_STATUS_NAMES.get(st, st)}")
    if assumptions is not None:
        if r["sat"]:
            return True, {abs(l): l > 0 for l in r["model"]}, None, None
        return False, None, proof_of_cdcl(r), list(r["core"])
    if r["sat"]:
        return True, {abs(l): l > 0 for l in r["model"]}, None
    return False, None, proof_of_cdcl(r)


def pysat_solver(formula: Formula) -> List[Assignment]:
    """REF.py:387-397 delegates to PySAT's Glucose3, a third-party clause-learning solver.
    It is used when installed; otherwise the library's own sound CDCL answers
    (cdcl_sound_solve), in PySAT's model shape: one dict over the variables
    1 .. max |literal|, those that do not occur False, or [] for UNSAT."""
    try:
        from pysat.formula import CNF
        from pysat.solvers import Solver
    except ImportError:
        sat, model, _ = cdcl_sound_solve(formula)
        if not sat:
            return []
        top = max((abs(l) for c in formula for l in c), default=0)
        return [{v: model.get(v, False) for v in range(1, top + 1)}]
    cnf = CNF()
    for clause in formula:
        cnf.append(clause)
    with Solver(name="glucose3", bootstrap_with=cnf) as solver:
        if solver.solve():
            return [{abs(lit): lit > 0 for lit in solver.get_model()}]
        return []


def cdcl_solve(formula: Formula) -> Tuple[bool, Optional[Assignment]]:
    """REF.py:382-384 on the GPU (csrc/cdcl.hip): the reference's CDCLSolver, same
    watch-list / dict / activity orders, so the same verdict and the same model
    dict.  The reference's loop can run forever; under the driver's deadline the
    call raises SolverTimeout like the other solvers."""
    from .cdcl import CdclLimit
    from .cdcl import cdcl_solve as _gpu_cdcl
    try:
        return _gpu_cdcl(formula, time_limit=_time_limit)
    except CdclLimit as e:
        raise SolverTimeout(f"Timeout after {_time_limit:g} seconds" if _time_limit else str(e)) from e


def hybrid_solver(formula: Formula, threshold=1000) -> List[Assignment]:
    """REF.py:400-404: PySAT above `threshold` clauses, DPLL below."""
    if len(formula) > threshold:
        return pysat_solver(formula)
    return dpll_optimized(formula)
