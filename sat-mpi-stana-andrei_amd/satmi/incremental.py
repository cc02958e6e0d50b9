"""An incremental solver in PySAT's shape over the sound CDCL on the GPU: a loop of
add_clause and solve(assumptions=...) on one growing formula, where every query starts with
the lemmas the queries before it learned (satmi_cdcl_carry_batch_host).

    with Solver(bootstrap_with=formula) as s:
        s.solve(assumptions=[4, -7])      # True / False / None (conflict_limit reached)
        s.get_core()                      # after False: the assumptions to blame
        s.solve(assumptions=[4, -7], minimal_core=True)     # ... and none of them a bystander
        s.add_clause([1, -3])
        s.solve()

Every lemma of the search follows from the formula alone, never from the assumptions, so it
holds for the next query under other assumptions and after clauses were added.  Clauses can
only be added: a lemma may rest on any clause of the formula, so after a removal the kept
lemmas would no longer follow and every later UNSAT answer would be unfounded.  A clause
that has to go later is added with a selector literal, [-s] + clause, and switched on by
assuming s."""
from . import _capi
from .cdcl_sound import cdcl_carry_batch, cdcl_shrink_batch

_SUMMED = ("conflicts", "decisions", "propagated", "rounds")


class Solver:
    def __init__(self, bootstrap_with=None, time_limit=0.0):
        self._clauses, self._lemmas = [], []
        self._time_limit = time_limit
        self._last, self._assumed = None, []
        self._stats = dict.fromkeys(_SUMMED, 0)
        self._stats["queries"] = 0
        if bootstrap_with is not None:
            self.append_formula(bootstrap_with)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.delete()
        return False

    def delete(self):
        """Forget the formula and the lemmas (PySAT's delete)."""
        self._clauses, self._lemmas, self._last = [], [], None

    def add_clause(self, clause):
        clause = [int(l) for l in clause]
        if any(l == 0 or not -2 ** 31 < l < 2 ** 31 for l in clause):
            raise ValueError("literals must be nonzero and within int32 (INT32_MIN excluded)")
        self._clauses.append(clause)

    def append_formula(self, formula):
        for c in formula:
            self.add_clause(c)

    def solve(self, assumptions=(), conflict_limit=0, minimal_core=False):
        """Is the formula satisfiable with every assumption true?  True, False, or None when
        conflict_limit > 0 conflicts did not decide it; the next call goes on from the lemmas
        learned so far in all three cases.  Raises SatmiError when the search could not run
        (the formula is beyond the kernel's layout, or the region's cap is reached).
        With `minimal_core` a False answer's core is shrunk in the same launch
        (satmi_cdcl_shrink_batch_host): the formula is satisfiable with the core less any one
        literal, unless a trial query reached conflict_limit and kept its literal unproven;
        the lemmas of every trial are kept, and accum_stats counts the trials."""
        self._assumed = [int(a) for a in assumptions]
        query = cdcl_shrink_batch if minimal_core else cdcl_carry_batch
        r = query([self._clauses], [self._assumed], [self._lemmas], conflict_limit=conflict_limit,
                             time_limit=self._time_limit)[0]
        self._last = None
        st = r["status"]
        if st in (_capi.CDCL_SOUND_TOO_LARGE, _capi.CDCL_SOUND_FULL):
            raise _capi.SatmiError(f"incremental.Solver: the search ended {_capi.CDCL_SOUND_STATUS_NAMES[st]}")
        self._lemmas = r["kept"]
        for k in _SUMMED:
            self._stats[k] += r["counters"][k]
        self._stats["queries"] += 1
        if minimal_core:
            self._stats["trials"] = self._stats.get("trials", 0) + r["shrink"]["queries"] - 1
        self._last = r
        return r["sat"]

    def get_model(self):
        """After True: one signed literal per variable of formula, lemmas and assumptions."""
        return list(self._last["model"]) if self._last and self._last["sat"] else None

    def get_core(self):
        """After False: the failed assumptions, the refuted one first ([]: the formula alone
        is unsatisfiable)."""
        return list(self._last["core"]) if self._last and self._last["sat"] is False else None

    def get_proof(self):
        """After False: (formula, lemmas) for refute.check_refutation: the current formula plus
        the core's literals as unit clauses, and every lemma kept so far with the empty clause
        last."""
        if not self._last or self._last["sat"] is not False:
            return None
        return ([list(c) for c in self._clauses] + [[l] for l in self._last["core"]],
                [list(c) for c in self._last["proof"]])

    def nof_clauses(self):
        return len(self._clauses)

    def nof_lemmas(self):
        return len(self._lemmas)

    def accum_stats(self):
        """Conflicts, decisions, propagated literals and rounds, summed over the calls (and
        "trials", the trial queries of the calls with minimal_core, once there was one)."""
        return dict(self._stats)
