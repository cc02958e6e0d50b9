"""CPU checks of the core-shrinking rule (tests/cdcl_shrink_rows.py) at its own rows: every core
that the chain proves minimal is unsatisfiable with the formula and satisfiable less any one
literal, it is a sublist of query 0's core, the region's records refute the formula plus the
core's units by plain reverse unit propagation (tests/refute_rows.py), and the same records
do not refute the formula plus the core less one literal."""
import functools

import cdcl_shrink_rows as S
import cdcl_sound_rows as R
import refute_rows as rr

ROWS = S.rows()
DONE = [r for r in ROWS if S.want(r)["status"] == S.ASSUMED and S.want(r)["shrink"][3] == 0]
BRUTE_MAX = 12      # variables up to which brute force decides; beyond, the sound rule of cdcl_sound_rows


def _units(lits):
    return [[l] for l in lits]


@functools.lru_cache(maxsize=None)
def _satisfiable(key):
    f = [list(c) for c in key]
    if len({abs(l) for c in f for l in c}) <= BRUTE_MAX:
        return R.brute_force(f)
    return R.solve(f)["status"] == R.SAT


def satisfiable(f):
    return _satisfiable(tuple(tuple(c) for c in f))


def test_rows_reach_every_end_of_a_chain():
    ends = {S.want(r)["status"] for r in ROWS}
    assert ends == {S.UNSAT, S.SAT, S.FULL, S.TOO_LARGE, S.ASSUMED}
    trials = {st for r in ROWS for _, st in S.want(r)["trials"]}
    assert trials == {S.UNSAT, S.SAT, S.LIMIT, S.FULL, S.ASSUMED}
    assert len(DONE) > 200 and any(S.want(r)["shrink"][3] for r in ROWS)
    assert max(S.want(r)["shrink"][0] for r in ROWS) >= 6
    assert any(r[3] for r in DONE) and any(max(map(len, r[1])) > R.SHORT_MAX for r in DONE)


def test_the_counts_add_up():
    for r in ROWS:
        w = S.want(r)
        q, sat, assumed, limit, first, zero = w["shrink"]
        ended = sum(st in (S.UNSAT, S.FULL) for _, st in w["trials"])
        assert q == 1 + sat + assumed + limit + ended == 1 + len(w["trials"]) and zero == 0, r[0]
        assert q - 1 <= first == (len(w["first"]["core"]) if w["first"]["status"] == S.ASSUMED else 0), r[0]
        if w["status"] == S.ASSUMED:
            assert sat + limit == len(w["core"]) and w["lemmas"][-1] == [] and [] not in w["kept"], r[0]
            assert w["records"] == len(w["lemmas"]) and w["words"] == R.region_words(w["lemmas"]), r[0]


def test_minimal_cores_against_brute_force():
    for r in DONE:
        f, core = r[1], S.want(r)["core"]
        assert not satisfiable(f + _units(core)), r[0]
        for x in core:
            assert satisfiable(f + _units([y for y in core if y != x])), (r[0], x)


def test_core_is_a_sublist_of_the_first_core():
    for r in DONE:
        w = S.want(r)
        it = iter(w["first"]["core"])
        assert all(x in it for x in w["core"]), r[0]       # in order, each once
        assert set(w["first"]["core"]) <= set(r[2]), r[0]


def test_region_refutes_the_core_and_nothing_less():
    for r in DONE:
        f, w = r[1], S.want(r)
        carried = len(r[3])     # (a carried lemma is the caller's claim: an earlier search's, RUP in its order)
        assert rr.evaluate(f + _units(w["core"]), w["lemmas"])[0][0] == rr.PROVEN, r[0]
        assert w["lemmas"][:carried] == r[3], r[0]
        for x in w["core"]:
            less = f + _units([y for y in w["core"] if y != x])
            assert rr.evaluate(less, w["lemmas"])[0][0] != rr.PROVEN, (r[0], x)


def test_unsat_trial_refutes_the_formula_alone():
    r = next(r for r in ROWS if r[0] == "unsat trial")
    w = S.want(r)
    assert w["status"] == S.UNSAT and w["core"] == [] and not satisfiable(r[1])
    assert rr.evaluate(r[1], w["lemmas"])[0][0] == rr.PROVEN
