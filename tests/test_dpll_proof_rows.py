"""CPU checks of the DPLL refutation rows (tests/dpll_proof_rows.py): the oracle decides
every row as the row's section says, and is_postorder accepts exactly the post-order walks
of decision trees."""
import functools

import oracle
import dpll_proof_rows as R
import refute_rows as rr


@functools.lru_cache(maxsize=None)
def decided():
    return {name: oracle.dpll(f, "sound", max_solutions=1, sol_cap=1) for name, f in R.all_rows()}


def _unsat(o):
    return o["status"] == 0 and o["counters"]["solutions"] == 0


def test_mixed_rows_hold_enough_unsat_searches_with_pure_literals():
    rows = R.mixed_rows()
    assert len(rows) == R.MIXED_COUNT
    for f in rows:
        assert 6 <= max(abs(l) for c in f for l in c) <= 14 and all(1 <= len(c) <= 4 for c in f)
    assert {len(c) for f in rows for c in f} == {1, 2, 3, 4}
    got = [decided()[f"mixed{s}"] for s in range(R.MIXED_COUNT)]
    unsat = [o for o in got if _unsat(o)]
    assert len(unsat) >= R.MIXED_UNSAT_MIN and len(unsat) < len(got)
    assert sum(o["counters"]["pure_assigns"] > 0 for o in unsat) >= R.MIXED_PURE_MIN
    assert sum(o["counters"]["decisions"] > 0 for o in unsat) >= 20


def test_ksat_rows_mix_verdicts_under_the_node_bound():
    got = [o for name, o in decided().items() if name.startswith("ksat")]
    assert len(got) == sum(r[3] for r in R.KSAT_ROWS)
    assert all(o["counters"]["nodes"] < R.KSAT_NODE_MAX for o in got)
    assert any(_unsat(o) for o in got) and any(o["counters"]["solutions"] for o in got)
    assert {(n, m) for n, m, _, _ in R.KSAT_ROWS} == {(20, 85), (20, 100), (50, 213), (50, 250)}


def test_bench_rows_are_unsat_under_the_node_bound():
    rows = R.bench_rows()
    assert len(rows) >= 3 and all(len(f) == 426 and max(abs(l) for c in f for l in c) <= 100 for f in rows)
    for i in range(len(rows)):
        o = decided()[f"bench{i}"]
        assert _unsat(o) and o["counters"]["nodes"] < R.BENCH_NODE_MAX


def test_hand_rows():
    assert [[]] in R.HAND_ROWS and [[1], [-1]] in R.HAND_ROWS
    assert any(len(set(c)) < len(c) for f in R.HAND_ROWS for c in f)                  # duplicate literals
    assert any(any(-l in c for l in c) for f in R.HAND_ROWS for c in f)               # tautologies
    assert max(len(c) for c in R.long_row()) == R.LONG_LEN > 255 and _unsat(decided()["long"])
    assert _unsat(decided()["hand1"]) and decided()["hand5"]["counters"]["solutions"] == 1


def test_deep_row_reaches_past_64_frames_in_a_small_tree():
    c = decided()["deep"]["counters"]
    assert _unsat(decided()["deep"]) and c["pure_assigns"] == 0
    # decisions = 2 x (frames of the deepest path): the chain is decided one variable per level
    assert c["decisions"] == 2 * (R.DEEP_CHAIN - 1) and c["decisions"] // 2 > 64
    assert c["conflicts"] == c["decisions"] // 2 + 1 and c["decisions"] + 1 < 2000


def test_unsat_rows_fix_the_conflict_count():
    """An exhausted search with no model: every decision node closes once, every leaf is a conflict."""
    for o in decided().values():
        if _unsat(o):
            c = o["counters"]
            assert c["conflicts"] == c["decisions"] // 2 + 1 and c["decisions"] % 2 == 0


QUAD2 = [[1, 2], [1, -2], [-1, 2], [-1, -2]]


def test_is_postorder_accepts_hand_made_trees():
    assert R.is_postorder([[]])
    assert R.is_postorder([[-1], [1], []])
    assert R.is_postorder([[-1, -2], [-1, 2], [-1], [1], []])
    assert R.is_postorder([[-3], [3, -1, -2], [3, -1, 2], [3, -1], [3, 1], [3], []])
    assert R.tree_depth([[-1, -2], [-1, 2], [-1], [1], []]) == 2


def test_is_postorder_rejects_what_is_no_walk():
    assert not R.is_postorder([[1], [-1], []])                    # a swapped pair: False before True
    assert not R.is_postorder([[-1], []])                         # a missing sibling
    assert not R.is_postorder([[-1, -2], [-1], [1], []])          # ... below the root
    assert not R.is_postorder([[-1], [1]])                        # no []
    assert not R.is_postorder([])
    assert not R.is_postorder([[-1], [1], [], []])                # something behind the root
    assert not R.is_postorder([[-1, -2], [1], []])                # a child two levels down
    assert not R.is_postorder([[-1, 1], [1], []])                 # a variable twice on a path


def test_evaluator_proves_a_hand_written_proof():
    words, ok = rr.evaluate(QUAD2, [[-1], [1], []])
    assert words == [rr.PROVEN, 0, -1, 0] and ok == [1, 1, 1]
    assert rr.evaluate(QUAD2[:3], [[-1], [1], []])[0][0] == rr.FAILED
