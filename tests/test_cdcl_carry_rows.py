"""CPU checks of the sound CDCL's rule with carried lemmas in Python (tests/cdcl_carry_rows.py):
with nothing carried it is cdcl_assume_rows.solve; chains of queries, each carrying the one
before's kept lemmas, are held to brute force and to a plain RUP check; a search cut by
conflict_limit and resumed ends with the uncut search's verdict; the rows reach every path."""
import functools

import pytest

import cdcl_assume_rows as A
import cdcl_carry_rows as C
import cdcl_sound_rows as R


def _units(lits):
    return [[l] for l in lits]


def test_with_an_empty_carry_it_is_the_assumption_rule():
    for name, f, a in A.rows():
        w, g = A.solve(f, a), C.solve(f, a)
        assert {k: g[k] for k in w} == w, name
        assert g["kept"] == [c for c in w["lemmas"] if c], name
        assert (g["records"], g["words"], g["flags"]) == (len(w["lemmas"]), R.region_words(w["lemmas"]), 0), name
    f = R.php(4)
    assert C.solve(f, [1, 6], 3)["lemmas"] == A.solve(f, [1, 6], 3)["lemmas"]


def test_chains_of_queries_equal_brute_force_and_their_proofs_check():
    count = {C.SAT: 0, C.UNSAT: 0, C.ASSUMED: 0}
    grown = carried = 0
    for queries in C.random_chains():
        assert 3 <= len(queries) <= 5
        kept, before = [], None
        for f, a in queries:
            assert max(abs(l) for c in f for l in c) <= 12
            grown += before is not None and len(f) > len(before)
            assert before is None or f[:len(before)] == before       # clauses are only added
            before = f
            r = C.solve(f, a, 0, kept)
            carried += bool(kept)
            count[r["status"]] += 1
            both = f + _units(a)
            assert (r["status"] == C.SAT) == R.brute_force(both), (f, a, kept)
            assert r["lemmas"][:len(kept)] == kept
            if r["status"] == C.SAT:
                assert R.satisfies(both, r["model"]) and r["core"] is None
                assert r["kept"] == r["lemmas"]
            else:
                core = r["core"]
                assert A.is_sublist(core, a) and (core == []) == (r["status"] == C.UNSAT), (f, a, core)
                assert r["lemmas"] == r["kept"] + [[]]
                assert A.refutes(f + _units(core), r["kept"] + [[]]), (f, a, kept)
                assert all(A.rup(f + r["kept"][:j], c) for j, c in enumerate(r["kept"]))      # each from F alone
            learned = dict(zip(C.COUNTERS, r["counters"]))["learned"]
            assert len(r["kept"]) == len(kept) + learned and r["records"] == len(r["lemmas"])
            kept = r["kept"]
    assert all(n >= 100 for n in count.values()), count
    assert grown >= 100 and carried >= 300, (grown, carried)


@pytest.mark.parametrize("name,f,a,limit", [
    ("php 5", R.php(5), [], 8),
    ("php 4 under assumptions", R.php(4), [1, 6, 11], 2),
    ("php 3 under six selectors",) + A.php_selector_row() + (3,),
    ("random 3-SAT 1", R.random_row()[1], [], 8),
    ("random 3-SAT 2 assumed", A.random_row()[2][0], A.random_row()[2][1], 5),
])
def test_a_search_cut_by_its_limit_and_resumed_gives_the_uncut_verdict(name, f, a, limit):
    whole = C.solve(f, a)
    last, slices = C.resume(f, a, limit)
    assert whole["status"] in (C.SAT, C.UNSAT, C.ASSUMED) and last["status"] == whole["status"], name
    assert slices >= 2, name
    if last["status"] == C.SAT:
        assert R.satisfies(f + _units(a), last["model"])
    else:
        assert A.is_sublist(last["core"], a)
        assert A.refutes(f + _units(last["core"]), last["lemmas"]), name


def test_php_5_in_slices_of_8_conflicts_is_unsat():
    last, slices = C.resume(R.php(5), (), 8)
    assert last["status"] == C.UNSAT and slices > 4 and A.refutes(R.php(5), last["lemmas"])


@functools.lru_cache(maxsize=None)
def _row_results():
    return {n: C.solve(f, a, C.LIMITS.get(n, 0), c, room, nv) for n, f, a, c, room, nv in C.rows()}


def test_rows_reach_every_path():
    """A condition on the rows, checked through the counters the restatement keeps."""
    res = _row_results()
    assert len(res) == len(C.rows())        # the names are distinct
    for hit in C.HITS:
        assert any(r["hits"][hit] for r in res.values()), hit
    got = [r["status"] for r in res.values()]
    for status in (C.SAT, C.UNSAT, C.ASSUMED, C.LIMIT, C.FULL, C.TOO_LARGE):
        assert status in got, status
    # and with a carry, not only without one
    with_carry = {res[n]["status"] for n, _, _, c, _, _ in C.rows() if c}
    assert with_carry == {C.SAT, C.UNSAT, C.ASSUMED, C.LIMIT, C.FULL, C.TOO_LARGE}


def test_rows_meet_their_conditions():
    res = _row_results()
    r = res["carried lemmas refute php 3 at level 0"]
    c = dict(zip(C.COUNTERS, r["counters"]))
    assert r["status"] == C.UNSAT and c["learned"] == 0 and c["decisions"] == 0 and c["conflicts"] == 1
    r = res["room equal to the carry: SAT"]
    assert r["status"] == C.SAT and r["model"] == [-1, 2, -3] and r["kept"] == [[1, 2, 3]]
    r = res["room equal to the carry: FULL"]
    assert r["status"] == C.FULL and r["flags"] == C.TRUNCATED and r["records"] == len(r["kept"]) + 1
    assert r["kept"] == C.solve(R.php(4), (), 4)["kept"]
    r = res["room one short of the closing record"]
    assert r["status"] == C.FULL and r["words"] == R.region_words(r["kept"]) + 1
    r = res["literal beyond inst_nvars with a carry"]
    assert (r["status"], r["flags"], r["kept"]) == (C.TOO_LARGE, 0, [[1]])
    for n in ("bogus: carried literal beyond inst_nvars", "bogus: carry larger than the room"):
        assert (res[n]["status"], res[n]["flags"], res[n]["kept"]) == (C.TOO_LARGE, C.BAD_CARRY, []), n
    assert res["limit with a carry"]["status"] == C.LIMIT and len(res["limit with a carry"]["kept"]) == 4
    for k in (1, 63, 64, 65):
        r = res[f"carried lemma of {k}"]
        assert r["status"] == C.SAT and k in r["model"] and r["kept"] == [list(range(1, k + 1))]
    r = res["carried clause over a new variable"]
    assert r["status"] == C.SAT and 7 in r["model"]


def test_malformed_carries_of_the_rule():
    for carry in ([[]], [[1], []], [[0]], [[C.I32_MIN]], [[3]]):
        r = C.solve([[1, 2]], (), 0, carry, None, 2)
        assert (r["status"], r["flags"], r["kept"], r["records"]) == (C.TOO_LARGE, C.BAD_CARRY, [], 0), carry


def test_a_bogus_carried_unit_makes_a_satisfiable_formula_unsat_and_the_check_rejects_it():
    _, f, a, carry, _, _ = next(r for r in C.rows() if r[0].startswith("bogus unit"))
    assert R.brute_force(f) and C.solve(f)["status"] == C.SAT
    r = C.solve(f, a, 0, carry)
    assert r["status"] == C.UNSAT and r["lemmas"] == carry + [[]]
    assert not A.refutes(f, r["lemmas"]) and not A.rup(f, carry[0])
