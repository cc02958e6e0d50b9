"""The selection of tests/cert_rows.py held to facts, on the CPU, so that
tests/test_cert_paths_gpu.py cannot silently shrink: every row has the verdict
and the sizes its table lists, fits the three certifier kernels' limits, and
the floors on rows, verdicts and clause lengths hold.  The negative cases are
proven here: a chain with any one of three clauses dropped has a model, shown in
plain Python; every False row is unsatisfiable by a plain DPLL search that shares
nothing with the oracle or the kernels (cert_rows.plain_unsat), beside the
oracle's own decision.  Rows are parametrised from the tables of cert_rows.py;
the oracle runs inside the tests."""
import pytest

import cert_rows as C
import refute_rows as rr
import res_paths
import trim_rows as tr
import witness_rows as wr
from satmi import _capi

DP_ROWS, RES_ROWS = C.dp_rows(), C.res_rows()


def test_limits_are_the_librarys():
    assert (C.TRIM_MAX_VARS, C.REFUTE_MAX_VARS, C.WITNESS_MAX_VARS) == \
        (_capi.TRIM_MAX_VARS, _capi.REFUTE_MAX_VARS, _capi.WITNESS_MAX_VARS) == (tr.MAX_VARS, rr.MAX_VARS, wr.MAX_VARS)
    assert C.SHORT_MAX == rr.SHORT_MAX == wr.SHORT_MAX


def test_davis_putnam_rows_are_the_table():
    assert sorted(DP_ROWS) == sorted(C.DP_TABLE)
    top = {"chain": [], "disjoint": []}
    for name in DP_ROWS:
        want_verdict, want_p, want_id, want_len = C.DP_TABLE[name]
        f, o = C.formula("dp", name), C.oracle_run("dp", name)
        rec = C.record(o)
        ids = C.variables(f + rec)
        assert o["result"] == want_verdict, name
        assert len(rec) == want_p, name
        if want_id is None:
            top[name.split("_")[0]].append(ids[-1])
        else:
            assert ids[-1] == want_id, name
        if want_len is None:
            assert C.longest("dp", name) in C.DISJOINT_LONGEST, name
        else:
            assert C.longest("dp", name) == want_len, name
    for group, (lo, hi) in C.DP_MAX_ID.items():
        assert (min(top[group]), max(top[group])) == (lo, hi), group
    assert {C.longest("dp", n) for n in DP_ROWS if n.startswith("disjoint")} == set(C.DISJOINT_LONGEST)


def test_resolution_rows_are_the_table():
    """Every row the fixture marks complete and keys_even; each formula is the one the reference
    ran on (cert_rows.formula asserts the hash); all eight answer True."""
    assert RES_ROWS == list(C.RES_TABLE)
    for name in ("chain30", "chain40", "stage_one_stripe", "stage_present", "keys_even", "abuf", "pairbuf", "pairbuf_wide"):
        assert name in RES_ROWS
    for name in RES_ROWS:
        o = C.oracle_run("res", name)
        assert (o["result"], len(C.record(o))) == C.RES_TABLE[name], name
        want = res_paths.row(name)[1]
        if want is not None:
            assert sorted(map(sorted, C.record(o))) == want, name


def test_every_row_fits_the_three_kernels():
    for kind, name in C.rows():
        f, rec = C.formula(kind, name), C.record(C.oracle_run(kind, name))
        top = C.variables(f + rec)[-1]
        assert top <= C.TRIM_MAX_VARS < C.REFUTE_MAX_VARS < C.WITNESS_MAX_VARS, name
        assert len(f) + len(rec) + 1 < 2 ** 31 and sum(map(len, f + rec)) < 2 ** 31


def test_floors():
    rows = C.rows()
    true = [r for r in rows if C.verdict(*r) == 1]
    false = [r for r in rows if C.verdict(*r) == 0]
    assert len(DP_ROWS) >= 24 and len(RES_ROWS) >= 8
    assert len(true) >= 10 and len(false) >= 10 and len(true) + len(false) == len(rows)
    lengths = {r: C.longest(*r) for r in false}
    assert any(n == C.SHORT_MAX for n in lengths.values())            # php65: the last length of the short form
    # no False row has a clause of 9 or more literals in formula or record (php65's longest
    # resolvents have 8; every row with longer clauses answers True: abuf, keys_even, pairbuf_wide,
    # stage_*), so that floor is left out; the wave-per-clause form runs on every False row all
    # the same, through max_clause_len = 0
    assert max(lengths.values()) == C.SHORT_MAX
    assert any(C.longest(*r) > C.SHORT_MAX for r in true)
    # every resolution path row answers True: proof_of_resolution meets False answers in the
    # batched lists only (res_edge, res_mix)
    assert all(C.verdict("res", n) == 1 for n in RES_ROWS)


def test_forward_rows():
    names = [n for _, n in C.forward_rows()]
    assert names == ["chain_64_unsat", "chain_65_unsat", "chain_128_unsat", "chain_129_unsat", "many_20", "php65"]


@pytest.mark.parametrize("name", C.chain_unsat_rows())
def test_a_chain_without_one_clause_has_a_model(name):
    """A chain is minimally unsatisfiable: without [x1] all False is a model, without [-xn] all
    True, without the link k -> k + 1 True up to xk and False behind it."""
    n, x = C.chain_parts(name)
    f = C.formula("dp", name)
    at = C.chain_positions(name)
    assert len(set(at)) == 3 and len(f) == n + 1
    assert (f[at[0]], f[at[1]], f[at[2]]) == ([x[1]], [-x[n]], [-x[n // 2], x[n // 2 + 1]])
    for which, i in enumerate(at):
        g = C.drop_clause(f, i)
        model = C.chain_model(name, which)
        assert len(g) == n and [abs(l) for l in model] == C.variables(f)
        assert C.satisfies(g, model), (name, which)
        assert not C.satisfies(f, model) and C.falsified(f, model) == [i]


def test_chain_rows_cover_every_size():
    assert C.chain_unsat_rows() == ["chain_%d_unsat" % n for n in C.CHAIN_SIZES]


@pytest.mark.parametrize("kind,name", C.table_rows(0), ids=lambda x: x)
def test_false_rows_are_unsatisfiable(kind, name):
    """By the plain search, which is independent; unsat_by_oracle beyond 20 variables is the
    oracle's Davis-Putnam again, so for a whole row it only shows that the function works."""
    assert C.verdict(kind, name) == 0 and (kind, name) not in C.UNSOUND_FALSE
    assert C.plain_unsat(C.formula(kind, name))
    assert C.unsat_by_oracle(C.formula(kind, name))


def test_the_tables_list_every_row():
    assert sorted(C.table_rows(0) + C.table_rows(1)) == sorted(C.rows())
    assert all(C.table(*r) == (C.verdict(*r), len(C.record(C.oracle_run(*r)))) for r in C.rows())


def test_unsound_false_is_empty():
    """No path row answers False for a satisfiable formula (the batched lists have such rows:
    test_batch_lists)."""
    got = [r for r in C.rows() if C.verdict(*r) == 0 and not C.plain_unsat(C.formula(*r))]
    assert got == C.UNSOUND_FALSE == []


def test_the_plain_references():
    assert C.satisfies([[1, -2], [2, 3]], [1, -2, 3]) and not C.satisfies([[1, -2], [2, 3]], [-1, 2, 3])
    assert not C.satisfies([[]], []) and C.satisfies([], []) and not C.satisfies([[4]], [1])
    assert C.falsified([[1], [-1], [2]], [1, -2]) == [1, 2]
    assert C.drop_clause([[1], [2], [3]], 1) == [[1], [3]]
    assert C.unsat_by_oracle([[1], [-1]]) and not C.unsat_by_oracle([[1, 2], [-1, 2]]) and not C.unsat_by_oracle([])
    assert C.unsat_by_oracle([[1, 2], []]) and not C.unsat_by_oracle([[1, -1]])
    assert C.unsat_by_oracle(rr.QUAD + [[-1]]) and not C.unsat_by_oracle(rr.QUAD)
    # the plain search against enumeration and against brute force, on small random formulas
    for f, p in rr.random_small(5, count=300):
        if not any(0 in c for c in f):
            assert C.plain_unsat(f) == C.unsat_by_oracle(f) == rr.implied(f, [], 5), f
    assert C.plain_unsat(rr.QUAD + [[-1]]) and not C.plain_unsat(rr.QUAD) and C.plain_unsat([[1, 2], []])
    # the plain propagation against tests/refute_rows.py's naive rounds, on its small random pairs
    for f, p in rr.random_small(3, count=300):
        if any(0 in c for c in f + p):
            continue
        _, oks = rr.evaluate(f, p)
        rup = C.Rup(f)
        for lemma, ok in zip(p, oks):
            if ok < 0:
                break
            assert rup.conflict(lemma) == bool(ok), (f, p)
            rup.add(lemma)
    for k in (1, 2, 64, 65):
        for f, p in rr.chain_cases(k):
            assert C.rup_conflict(f, p[0]) == bool(rr.evaluate(f, p)[1][0])


@pytest.mark.parametrize("name", ["many_20", "chain_64_unsat", "chain_129_unsat", "chain_300_unsat"])
def test_the_oracles_record_is_a_refutation_in_plain_python(name):
    """What the GPU test asks of the kernels' records holds of the oracle's: the whole record
    with [] appended passes the plain forward check, and fails it with a chain clause dropped."""
    f = C.formula("dp", name)
    proof = C.record(C.oracle_run("dp", name)) + [[]]
    assert C.rup_proof(f, proof)
    if name.startswith("chain"):
        for i in C.chain_positions(name):
            assert not C.rup_proof(C.drop_clause(f, i), proof)


@pytest.mark.parametrize("name", list(C.batch_rows()))
def test_batch_lists(name):
    """Both verdicts occur in every list; the answers that are wrong are exactly the listed ones."""
    kind, fs, cap = C.batch_rows()[name]
    v = C.batch_verdicts(name)
    assert len(v) == len(fs) and set(v) == {0, 1}
    assert (v.count(1), v.count(0)) == C.BATCH_COUNTS[name]
    assert C.batch_unsound(name) == C.BATCH_UNSOUND.get(name, ((), ()))
    for b in C.batch_unsound(name)[0]:
        assert [] in fs[b]
    for b in C.batch_unsound(name)[1]:
        assert any(-l in c for c in fs[b] for l in c)
