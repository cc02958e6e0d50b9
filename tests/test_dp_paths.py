"""CPU checks of tests/dp_paths.py: every row has the dense variable count and
the key width it is named for, the oracle finishes it within its step limit
(no clause limit, no time limit), and the rows that are there for a size --
a list length, a pair count, a resume -- have that size in the oracle's
record.  A later edit of a seed cannot move a row back into the one layout
class (K = 2, everything in LDS) the rest of the suite runs in."""
import pytest

import dp_paths as P


@pytest.mark.parametrize("name", list(P.ROWS))
def test_row_shape_and_oracle(name):
    _, step_limit, V = P.ROWS[name]
    f, o = P.row_formula(name), P.row_oracle(name)
    assert len(P.variables(f)) == V
    if step_limit == 0:   # to the verdict; the step that found the empty resolvent is not recorded
        assert o["result"] in (0, 1)
        assert len(o["clauses"]) == o["steps"] - (o["result"] == 0)
    else:                 # every step up to the limit completed and recorded
        assert o["result"] == -1 and o["steps"] == step_limit == len(o["clauses"])
    assert sum(len(c) for s in o["clauses"] for c in s) < 1 << 22   # the record's capacity


def test_key_widths():
    want = {64: 2, 65: 4, 128: 4, 129: 6, 192: 6, 193: 8, 256: 8, 257: 10, 70: 4, 130: 6, 200: 8, 260: 10}
    seen = set()
    for name in P.KEY_WIDTH_ROWS:
        V = P.ROWS[name][2]
        assert P.key_words(V) == want[V], name
        seen.add(P.key_words(V))
    assert seen == {2, 4, 6, 8, 10}
    for V in (64, 65, 128, 129, 192, 193, 256, 257):
        for kind in ("sparse3_%d_x37", "sparse3_%d_x1", "chain_%d_sat", "chain_%d_unsat"):
            assert kind % V in P.ROWS
        assert P.row_oracle("chain_%d_sat" % V)["result"] == 1
        assert P.row_oracle("chain_%d_unsat" % V)["result"] == 0


@pytest.mark.parametrize("name", [n for n in P.ROWS if n.endswith("_x37") or n.startswith(("popset", "chain", "long_70", "long_200"))])
def test_sparse_ids_build_the_set(name):
    """ids times 37: some id is not below the variable set's table size at the
    first pop, so pop() is decided by the insertion order, not the smallest id."""
    vs = P.variables(P.row_formula(name))
    assert max(vs) >= P.py_size_after(len(vs))


@pytest.mark.parametrize("name", [n for n in P.ROWS if n.endswith("_x1")] + list(P.LARGE_ROWS))
def test_small_ids_take_the_shortcut(name):
    vs = P.variables(P.row_formula(name))
    assert max(vs) < P.py_size_after(len(vs))
    assert P.row_oracle(name)["vars"][0] == min(vs)


@pytest.mark.parametrize("name", ["long_70", "long_200"])
def test_long_clause_rows(name):
    f = P.row_formula(name)
    dense = {v: d for d, v in enumerate(sorted(P.variables(f)))}
    long_ = [c for c in f if len(c) >= 20]
    assert len(long_) == 6 and all(20 <= len(c) <= 40 for c in long_)
    bounds = (64, 128) if name == "long_200" else (64,)
    for b in bounds:   # clauses with literals on both sides of the word boundary
        assert sum(1 for c in long_ if {b - 1, b} <= {dense[abs(l)] for l in c}) >= 2
    taut = [c for c in f if any(-l in c for l in c)]
    assert len(taut) == 1 and {dense[abs(l)] for l in taut[0] if -l in taut[0]} == {64}
    assert sum(1 for i, c in enumerate(f) if c in f[:i]) == 1   # the duplicate clause
    # a long clause is resolved within the step limit: tables past the assembly's LDS scratch
    assert max(max(s[4], s[5]) for s in P.step_sizes(name)) >= 20


def test_placement_rows():
    assert [P.cap_for(V) <= 2048 for V in (255, 256)] == [True, False]   # the model set: LDS / global scratch
    assert {P.ROWS[n][2] for n in P.POPSET_ROWS} == {255, 256, 300}
    assert {P.ROWS[n][2] for n in P.FIRSTPOS_ROWS} == {2048, 2049}        # the first-position table: LDS / global
    assert len(P.FIRSTPOS_ROWS) == 5


def test_large_list_rows():
    n = {name: [len(P.row_formula(name))] + [len(s) for s in P.row_oracle(name)["clauses"]] for name in P.LARGE_ROWS}
    assert all(16384 < x < 65536 for x in n["list_20000"][:3])    # runs of more than 16 clauses, the packed scan
    assert all(x >= 65536 for x in n["list_70000"][:3])           # the three-scan branch
    assert all(x >= 65536 for x in n["wide_pairs"][:2])
    s = P.step_sizes("wide_pairs")
    assert P.row_oracle("wide_pairs")["vars"][:2] == [1, 2]
    assert s[0][:2] == (300, 300) and 800 < s[0][3] <= 900       # (a few of the 900 repeat)
    assert s[1][0] == 0 and s[1][1] == s[0][3]                    # an empty pos list
    s = P.step_sizes("packed_sign")
    assert n["packed_sign"][0] < 65536 and s[0][0] == 1 and s[0][1] >= 1 << 15 and s[0][3] == 50


def test_width_change_sequence():
    Ks = [P.key_words(P.ROWS[n][2]) for n in P.WIDTH_CHANGE_SEQUENCE]
    assert Ks == [2, 4, 10, 2, 6, 2]
    assert all(P.ROWS[n][1] == 0 for n in P.WIDTH_CHANGE_SEQUENCE)          # each reaches its verdict
    assert max(a * b for a, b, *_ in P.step_sizes("many_20")) >= 500        # many resolvents per step


def test_resume_rows_force_their_resumes():
    for name, bits in P.RESUME_ROWS.items():
        assert P.forced_resumes(name) == set(bits), name
    assert {b for bits in P.RESUME_ROWS.values() for b in bits} == set(P.RESUME_KEYS)
    assert max(len(s) for s in P.row_oracle("php65")["clauses"]) > 3 * 1024 // 2
