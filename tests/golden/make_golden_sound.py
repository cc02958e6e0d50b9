"""Golden vectors for the BENCHMARKED DPLL semantics (SATMI_MODE_SOUND), made by
running the REFERENCE's own dpll_optimized with one statement rewritten.

Run here (the container that holds /root/reference):
    python tests/golden/make_golden_sound.py [--jobs 8] [--n100 48]

REF.py's dpll_optimized (REF.py:133-214) never applies a branch to the formula:
its branch loop (REF.py:210-213) copies the assignment, sets `var`, and recurses
on the *unreduced* formula.  SOUND mode applies the branch as a unit clause.
This script makes exactly that change, and only it, with an `ast` transform of
the loop body:

    new_assignment = assignment.copy()                      (kept)
    new_assignment[var] = val              ->  branch_lit = var if val else -var
    solutions.extend(dpll_optimized(formula, new_assignment))
                                           ->  solutions.extend(dpll_optimized(formula + [[branch_lit]], new_assignment))

so the branch literal reaches the child as the clause `[branch_lit]` and the
child assigns it with the reference's own unit_propagate (REF.py:139-165).
unit_propagate, pure-literal elimination (REF.py:174-195) and the variable
choice (REF.py:198-208) run unmodified.  The rewritten statements keep their
line numbers.

Counters are observed with `sys.settrace` (read-only), as in make_golden.py:
    nodes         calls of dpll_optimized
    decisions     executions of the `branch_lit = ...` line (REF.py:212)
    unit_props    executions of `a[var] = val` (REF.py:154) minus the decision
                  literals' own assignments: the appended clause [branch_lit]
                  is the only unit clause of a decision child's formula (the
                  parent's unit_propagate left none), so every decision child
                  assigns it exactly once, first -- the tracer asserts that
    pure_assigns  executions of `new_assignment[abs(lit)] = lit > 0` (REF.py:189)
    conflicts     executions of the `return []` after the root unit_propagate (REF.py:169)
The first model is the assignment dict at the first execution of a
`return [assignment]` (REF.py:171 / :206); the counters at that moment are the
counters of a search that stops at its first model (the bench's SAT/UNSAT
decision, max_solutions=1).  When the full enumeration finishes within the time
budget, its counters and solution count are recorded too.

Instances: edge formulas, the reference's generator (REF.py:21-29) driven by
`random`, and uniform random 3-SAT drawn with satmi.cnf.uniform_ksat (numpy, the
bench's own generator) at BASELINE configs[1] (n=50, alpha=4.26) and configs[2]
(n=100, alpha=4.26).  Output: tests/golden/dpll_sound_ref.json (plain data).
"""
import argparse
import ast
import json
import multiprocessing as mp
import os
import random
import signal
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_FILE = "/root/reference/comparatie intre algoritmii de rezolvare a seturilor de clauze.py"
OUT = os.path.join(HERE, "dpll_sound_ref.json")
WANTED = ("generate_large_formula", "dpll_optimized")


class _SoundBranch(ast.NodeTransformer):
    """Rewrite the two statements of dpll_optimized's `for val in [True, False]`
    body described in the module docstring; everything else is untouched."""

    def __init__(self):
        self.done = 0

    def visit_For(self, node):
        self.generic_visit(node)
        if not (isinstance(node.target, ast.Name) and node.target.id == "val"):
            return node
        body = []
        for st in node.body:
            txt = ast.unparse(st)
            if txt == "new_assignment[var] = val":
                new = ast.parse("branch_lit = var if val else -var").body[0]
                body.append(ast.copy_location(new, st))
                ast.fix_missing_locations(new)
                for sub in ast.walk(new):
                    sub.lineno, sub.end_lineno = st.lineno, st.end_lineno
                self.done += 1
            elif txt == "solutions.extend(dpll_optimized(formula, new_assignment))":
                new = ast.parse("solutions.extend(dpll_optimized(formula + [[branch_lit]], new_assignment))").body[0]
                for sub in ast.walk(new):
                    sub.lineno, sub.end_lineno = st.lineno, st.end_lineno
                    sub.col_offset, sub.end_col_offset = getattr(st, "col_offset", 0), getattr(st, "end_col_offset", 0)
                body.append(new)
                self.done += 1
            else:
                body.append(st)
        node.body = body
        return node


def load_reference():
    src = open(REF_FILE, encoding="utf-8").read()
    tree = ast.parse(src)
    body = []
    for node in tree.body:
        if isinstance(node, ast.Import):
            body.append(node)
        elif isinstance(node, ast.ImportFrom) and not node.module.startswith("pysat"):
            body.append(node)   # PySAT (REF.py:6-7) is absent and unused by these functions
        elif isinstance(node, ast.Assign):
            body.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name in WANTED:
            if node.name == "dpll_optimized":
                tr = _SoundBranch()
                node = tr.visit(node)
                assert tr.done == 2, "branch statements of REF.py:210-213 not found"
            body.append(node)
    ns = {"__name__": "reference_functions_sound"}
    exec(compile(ast.Module(body=body, type_ignores=[]), REF_FILE, "exec"), ns)
    lines = {}
    for fn in ast.walk(ast.parse(src)):   # the unmodified tree
        if isinstance(fn, ast.FunctionDef) and fn.name == "dpll_optimized":
            for st in ast.walk(fn):
                if isinstance(st, (ast.Assign, ast.Return, ast.Expr)):
                    lines.setdefault(ast.unparse(st), []).append(st.lineno)
    return ns, lines, src.splitlines()


NS, LINES, SRC = load_reference()
L_UNIT = LINES["a[var] = val"][0]
L_PURE = LINES["new_assignment[abs(lit)] = lit > 0"][0]
L_DEC = LINES["new_assignment[var] = val"][0]          # now `branch_lit = ...`, same line
L_SOL = set(LINES["return [assignment]"])              # REF.py:171 and :206
L_CONF = next(ln for ln in range(LINES["(formula, assignment) = unit_propagate(formula, assignment)"][0],
                                 LINES["(formula, assignment) = unit_propagate(formula, assignment)"][0] + 4)
              if SRC[ln - 1].strip() == "return []")
CODE = NS["dpll_optimized"].__code__


class Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise Timeout()


class _First(Exception):
    pass


def run_sound(formula, seconds, init=None, sol_cap=0, first_only=False):
    """Run the rewritten reference DPLL on `formula`; returns the observation.
    `init`: a caller's assignment dict, passed as the reference's second
    argument (the dict as the call leaves it is recorded as "init_after");
    `sol_cap` > 0: the first sol_cap solutions of a finished enumeration are
    kept, each in its dict order; `first_only`: the run is stopped by the
    observer at the first `return [assignment]`."""
    ctr = {"nodes": 0, "unit_raw": 0, "pure_assigns": 0, "decisions": 0, "conflicts": 0}
    first = {}
    pending = [0]   # decision children whose first unit assignment is still to come

    def snapshot():
        return {"nodes": ctr["nodes"], "decisions": ctr["decisions"],
                "unit_props": ctr["unit_raw"] - ctr["decisions"], "pure_assigns": ctr["pure_assigns"],
                "conflicts": ctr["conflicts"]}

    def local(frame, event, arg):
        if event != "line":
            return local
        ln = frame.f_lineno
        if ln == L_UNIT:
            ctr["unit_raw"] += 1
            if pending[0]:
                # the decision child's first assignment must be its branch literal
                lit = frame.f_locals["lit"]
                assert lit == pending[0], ("decision literal not assigned first", lit, pending[0])
                pending[0] = 0
        elif ln == L_PURE:
            ctr["pure_assigns"] += 1
        elif ln == L_DEC and frame.f_code is CODE:
            ctr["decisions"] += 1
        elif ln == L_CONF and frame.f_code is CODE:
            ctr["conflicts"] += 1
        elif ln in L_SOL and frame.f_code is CODE and not first:
            first["counters"] = snapshot()
            first["model"] = [v if b else -v for v, b in frame.f_locals["assignment"].items()]
            if first_only:
                raise _First()
        return local

    def glob(frame, event, arg):
        if event == "call" and frame.f_code is CODE:
            ctr["nodes"] += 1
            par = frame.f_back
            if par is not None and par.f_code is CODE and "branch_lit" in par.f_locals:
                pending[0] = par.f_locals["branch_lit"]
            return local
        if event == "call" and frame.f_code.co_filename == REF_FILE:
            return local
        return None

    f_copy = [list(c) for c in formula]
    args = () if init is None else (init,)
    signal.signal(signal.SIGALRM, _alarm)
    signal.setitimer(signal.ITIMER_REAL, seconds, 1.0)   # again every second: a raise that lands where CPython drops it must not leave the run unbounded
    sys.settrace(glob)
    done = True
    try:
        res = NS["dpll_optimized"](f_copy, *args)
    except (Timeout, _First):
        done = False
        res = None
    finally:
        sys.settrace(None)
        signal.setitimer(signal.ITIMER_REAL, 0)
    case = {"formula": formula}
    if first:
        case["first"] = {"counters": first["counters"], "model": first["model"]}
    elif done:   # UNSAT: the whole search is the first-model search
        case["first"] = {"counters": snapshot(), "model": None}
    if done:
        case["full"] = {"counters": snapshot(), "solutions": len(res),
                        "first_solution": ([v if b else -v for v, b in res[0].items()] if res else None)}
        if sol_cap > 0:
            case["full"]["solution_list"] = [[v if b else -v for v, b in s.items()] for s in res[:sol_cap]]
        if init is not None:
            case["init_after"] = [v if b else -v for v, b in init.items()]
    return case


def _job(args):
    formula, seconds, tag = args
    c = run_sound(formula, seconds)
    c["tag"] = tag
    return c


EDGE = [
    [], [[1]], [[-1]], [[1], [-1]], [[1, -1]], [[1, 1]], [[1, 1], [-1]],
    [[1, 2], [-1, 2], [1, -2], [-1, -2]], [[1], [-1, 2], [-2, 3, 4]], [[1], [1], [-1, 2]],
    [[2], [1, -2], [-1, 3], [-3, -2]], [[1, 2, 3]], [[-1, -2], [-2, -3], [-1, -3]],
    [[1, 2], [-2, 3], [-3, 1], [4, -4]], [[5, -3], [3, 1], [-1, -5, 2], [2, 4], [-4, -2, 3], [1]],
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--n50", type=int, default=96)
    ap.add_argument("--n100", type=int, default=48)
    ap.add_argument("--seconds", type=float, default=240.0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "sat-mpi-stana-andrei_amd"))
    from satmi import cnf

    jobs = [(f, 30.0, "edge") for f in EDGE]
    for seed in range(40):                          # the reference's own generator (REF.py:21-29)
        random.seed(5000 + seed)
        nclauses = random.randint(3, 60)
        maxlit = random.randint(1, 5)
        nvars = random.randint(max(maxlit, 2), 14)
        jobs.append((NS["generate_large_formula"](nclauses, maxlit, nvars), 30.0, "generator"))
    b50 = cnf.uniform_ksat(a.n50, 50, 213, 3, seed=50_2026)
    jobs += [(b50.instance(i), a.seconds, "configs1_n50") for i in range(a.n50)]
    b100 = cnf.uniform_ksat(a.n100, 100, 426, 3, seed=100_2026)
    jobs += [(b100.instance(i), a.seconds, "configs2_n100") for i in range(a.n100)]
    with mp.Pool(a.jobs) as pool:
        cases = pool.map(_job, jobs, chunksize=1)
    missing = [c["tag"] for c in cases if "first" not in c]
    meta = {"generator": "tests/golden/make_golden_sound.py", "python": sys.version.split()[0],
            "reference": os.path.basename(REF_FILE),
            "semantics": "REF.py dpll_optimized with the branch of REF.py:210-213 applied as a unit clause",
            "uniform_seeds": {"configs1_n50": [a.n50, 50, 213, 3, 50_2026],
                              "configs2_n100": [a.n100, 100, 426, 3, 100_2026]},
            "timed_out_first_model": len(missing)}
    cases = [c for c in cases if "first" in c]
    with open(OUT, "w") as fh:
        json.dump({"meta": meta, "cases": cases}, fh, separators=(",", ":"))
    by = {}
    for c in cases:
        by.setdefault(c["tag"], [0, 0])
        by[c["tag"]][0] += 1
        by[c["tag"]][1] += "full" in c
    print(OUT, len(cases), by, "timed out:", missing)


if __name__ == "__main__":
    main()
