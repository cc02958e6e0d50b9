"""CPU checks of the sound CDCL's path rows (tests/cdcl_sound_paths.py): every row takes, on the
Python rule, the path it is there for; at the rows that halve the activities a rule that halves
otherwise gives other words, so a kernel that did would be told from the rule; the rule's
answers at the rows are sound; and the four restatements agree where their inputs coincide."""
import pytest

import cdcl_assume_rows as A
import cdcl_carry_rows as C
import cdcl_shrink_rows as S
import cdcl_sound_paths as P
import cdcl_sound_rows as R

NAMES = [r[0] for r in P.rows()]


def _units(lits):
    return [[l] for l in lits]


def _words(r):
    """What the kernel is compared on, of a result of any restatement."""
    return r["status"], r["counters"], r["lemmas"], r["model"], r.get("core")


def test_every_row_is_named_once_and_has_its_needs():
    assert len(set(NAMES)) == len(NAMES) and set(NAMES) == set(P.NEEDS)
    reached = {k for n in NAMES for k in P.NEEDS[n]}
    assert reached == set(R.PATHS)              # every path has a row
    assert set(P.CHAIN_ROWS) <= set(P.HALVING_ROWS) and len(P.HALVING_ROWS) == 4


@pytest.mark.parametrize("name", NAMES)
def test_row_takes_its_path(name):
    """The witnesses: a row that stops taking its path fails here, not silently."""
    got = P.paths_of(name)
    for k, least in P.NEEDS[name].items():
        assert got[k] >= least >= P.PATH_REACHED[k], (name, k, got[k])


def test_the_rows_counters_are_the_ones_they_were_written_for():
    w = P.want("php 6")
    assert (w["status"], w["counters"][0], len(w["lemmas"]), w["paths"]["halvings"]) == (R.UNSAT, 284, 284, 1)
    w = P.want("two halvings")
    assert (w["status"], w["counters"][0], w["paths"]["halvings"]) == (R.UNSAT, 672, 2)
    assert max(abs(l) for c in P.row("two halvings")[1] for l in c) == 80      # a search over two 64-lane steps
    w = P.want("uip gap")
    assert w["counters"] == [1, 72, 74, 77, 1, 1, 71, 0] and w["lemmas"] == [[1]] and w["status"] == R.SAT
    assert P.want("uip gap to the decision")["lemmas"] == [[2, 1]] == P.want("low gap")["lemmas"]
    assert P.want("uip gap to the decision")["paths"]["collection walk gap"] == 0
    assert P.want("low gap")["paths"]["first-UIP walk gap"] == 0
    w = P.want("level 300")
    assert w["counters"] == [1, 301, 2, 305, 1, 300, 300, 0] and w["lemmas"] == [list(range(300, 0, -1))]
    w = P.want("final gap")
    assert w["status"] == A.ASSUMED and w["core"] == [80, 1] and w["counters"][0] == 0
    for name in NAMES:
        if name.startswith("opposite offers"):
            w = P.want(name)
            assert w["status"] == R.SAT and w["lemmas"] == [[1]] and w["counters"][0] == 1, name
    lens = [max(map(len, P.row(n)[1])) for n in NAMES if n.startswith("opposite offers")]
    assert sorted(lens) == [2, 2, 12] and R.SHORT_MAX < 12


def test_the_chain_rows_put_the_halving_where_they_say():
    """`php 6 under selectors`: query 0 is the search that halves, and seven SAT trials follow.
    `hard trial`: query 0 ends ASSUMED without a conflict, and the trial that drops 50, which
    starts with the region's re-walk, is the one that crosses 256 conflicts."""
    w = P.want("php 6 under selectors", "shrink")
    assert w["status"] == S.ASSUMED and w["shrink"] == [8, 7, 0, 0, 7, 0] and sorted(w["core"]) == P.PHP6_SELECTORS
    assert [(q["status"], q["counters"][0], q["paths"]["halvings"]) for q in w["queries"]] == \
        [(S.ASSUMED, 284, 1)] + [(S.SAT, 0, 0)] * 7
    w = P.want("hard trial", "shrink")
    assert w["status"] == S.ASSUMED and w["shrink"] == [9, 7, 1, 0, 8, 0] and sorted(w["core"]) == P.PHP6_SELECTORS
    assert w["first"]["core"][0] == P.TRIAL_SELECTOR and w["trials"][0] == (P.TRIAL_SELECTOR, S.ASSUMED)
    assert [(q["status"], q["counters"][0], q["paths"]["halvings"]) for q in w["queries"]] == \
        [(S.ASSUMED, 0, 0), (S.ASSUMED, 284, 1)] + [(S.SAT, 0, 0)] * 7


def test_resumed_halves_nowhere_and_a_count_carried_over_would():
    """LIMIT at 200 conflicts, then 204 more to UNSAT: the sum passes 256 and neither part does.
    By the rule a resumed search counts afresh; one that went on counting would halve at its
    56th conflict, and learns other clauses from there."""
    first, second = P.want("resumed: the first slice"), P.want("resumed")
    assert (first["status"], first["counters"][0]) == (C.LIMIT, P.RESUME_AT)
    assert (second["status"], second["counters"][0]) == (C.UNSAT, 204) and P.row("resumed")[3] == first["kept"]
    assert first["paths"]["halvings"] == second["paths"]["halvings"] == 0
    _, f, a, carry, limit = P.row("resumed")
    other = C.solve(f, a, limit, carry, conflicts_before=P.RESUME_AT)
    assert other["paths"]["halvings"] >= 1
    assert (other["counters"], other["lemmas"]) != (second["counters"], second["lemmas"])
    assert other["lemmas"][:len(carry) + 56] == second["lemmas"][:len(carry) + 56]


@pytest.mark.parametrize("variant", sorted(R.NOT_THE_RULE))
@pytest.mark.parametrize("name", P.HALVING_ROWS)
def test_another_halving_gives_other_words(name, variant):
    """No halving, a halving at conflicts % 256 == 255, one that rounds up: each gives
    another counter vector or lemma list than the rule at every halving row, so the comparison
    of tests/test_cdcl_sound_paths_gpu.py tells a kernel with that halving from the rule."""
    _, f, a, carry, limit = P.row(name)
    if name in P.CHAIN_ROWS:
        w, g = P.want(name, "shrink"), S.solve(f, a, limit, carry, halve=R.NOT_THE_RULE[variant])
    else:
        w, g = P.want(name), C.solve(f, a, limit, carry, halve=R.NOT_THE_RULE[variant])
    assert (g["counters"], g["lemmas"]) != (w["counters"], w["lemmas"]), (name, variant)
    if name == "php 6":     # the sound and the assume restatement have the same keyword, to the same effect
        assert _words(R.solve(f, limit, halve=R.NOT_THE_RULE[variant]))[:4] == _words(g)[:4]
        assert _words(A.solve(f, a, limit, halve=R.NOT_THE_RULE[variant])) == _words(g)


def test_the_default_keywords_are_the_rule():
    f = P.row("php 6")[1]
    assert R.HALVE == (256, 0, 0) and R.HALVE not in R.NOT_THE_RULE.values()
    assert _words(R.solve(f, halve=R.HALVE)) == _words(P.want("php 6", "sound"))
    assert _words(C.solve(f, halve=R.HALVE, conflicts_before=0)) == _words(P.want("php 6"))


def test_the_restatements_agree_at_the_rows():
    """Without assumptions and carry the four are one rule; the witnesses included.  (`two
    halvings` is left to the carrying restatement alone for its cost: what it adds to `php 6`, a
    second halving and ids past 64, goes through the same lines of all four.)"""
    for name in NAMES:
        if name == "two halvings":
            continue
        _, f, a, carry, limit = P.row(name)
        c = P.want(name)
        if not carry:
            s = P.want(name, "assume")
            assert {k: c[k] for k in s} == s, name
            if not a:
                r = P.want(name, "sound")
                assert {k: s[k] for k in r} == r, name
        if not a:
            s = S.solve(f, a, limit, carry)
            assert _words(s) == _words(c) and s["shrink"] == [1, 0, 0, 0, 0, 0], name
    assert _words(P.want("php 6", "sound"))[:4] == _words(P.want("php 6"))[:4]


def test_renamed_rows_are_their_originals_under_the_map():
    """The map is monotone, so the rule decides, implies and learns the same: equal counters, the
    lemmas and the model renamed.  Four of the rows are SAT and four UNSAT."""
    rand = R.random_row()
    status = []
    for i in P.RENAMED:
        w, g = R.solve(rand[i]), P.want(f"renamed {i}", "sound")
        assert g["status"] == w["status"] and g["counters"] == w["counters"], i
        assert g["lemmas"] == P.renamed(w["lemmas"]), i
        assert g["model"] == (P.renamed([w["model"]])[0] if w["model"] else None), i
        ids = sorted({abs(l) for c in P.row(f"renamed {i}")[1] for l in c})
        assert ids[0] >= 65 and ids[-1] == 261 and all(v % 4 == 1 for v in ids), i
        assert w["counters"][0] >= 30, i       # activities that differ, well before the end
        status.append(w["status"])
    assert status.count(R.SAT) == 4 and status.count(R.UNSAT) == 4


@pytest.mark.parametrize("name", NAMES)
def test_the_rules_answer_is_sound(name):
    """UNSAT and ASSUMED: the lemma list, the carried lemmas in front, is a refutation by reverse
    unit propagation of the formula and the core's units (the carry of `resumed` is the first
    slice's lemma list, RUP from the formula itself).  SAT: the model satisfies the formula."""
    _, f, a, carry, limit = P.row(name)
    w = P.want(name, "shrink") if name in P.CHAIN_ROWS else P.want(name)
    if w["status"] in (C.UNSAT, C.ASSUMED):
        assert A.is_sublist(w["core"], a), name
        assert A.refutes(f + _units(w["core"]), w["lemmas"]), name
    elif w["status"] == C.SAT:
        assert R.satisfies(f + _units(a), w["model"]), name
    else:
        assert (name, w["status"]) == ("resumed: the first slice", C.LIMIT)
        db = [list(c) for c in f]
        for c in w["lemmas"]:
            assert A.rup(db, c), name
            db.append(c)
