"""Formulas that drive the sound CDCL's kernels (csrc/cdcl_sound_search.inc, compiled as the
sound, the assumption-carrying, the lemma-carrying and the shrinking kernel) down the paths
that no row of cdcl_sound_rows, cdcl_assume_rows, cdcl_carry_rows or cdcl_shrink_rows enters,
shared by tests/test_cdcl_sound_paths.py (CPU: the rule's "paths" witnesses prove every row
takes the path it is there for, and a rule with another halving gives other words) and
tests/test_cdcl_sound_paths_gpu.py (GPU: every row word for word against the rule, through all
four entry points and in both clause forms).

The paths, in the kernel's terms, and the witness of cdcl_sound_rows.PATHS that proves each:

  * `if ((conflicts & 255) == 0) ... w.act[v] >>= 1`: "halvings".  The rows of the other modules
    end within 146 conflicts.
  * the decision key `act << 15 | (32767 - v)` over several `v0 += 64` steps with activities
    that differ, the model row's compaction over `__ballot(occ)` with gaps in the ids, the
    `seen` words beyond word 1: "decisions past lane 63 by activity" (a variable above 64 was
    decided while a lower id was unassigned: its activity won).
  * `idx -= 64` in the first-UIP walk: "first-UIP walk gap", the most unmarked trail entries
    between two marked ones; from 64 on the walk's first 64-entry window is empty.
  * the collection of the learned clause's lower literals, `bj` read in a later step than the
    first (`k == 0` there): "collection walk gap", the unmarked entries between the first UIP
    and the first lower literal.
  * `idx -= 64` in the final analysis under assumptions: "final walk gap".
  * `w.level`, 16 bits: "deepest level" past 255.
  * two unit clauses of one round that imply v and -v: the lower clause's offer stands (the
    short form's atomicMin within a 64-clause step, `win` across steps, the long form's first
    come) and the other clause is falsified in the next round: "opposite offers lost".
"""
import functools

import cdcl_assume_rows as A
import cdcl_carry_rows as C
import cdcl_shrink_rows as S
import cdcl_sound_rows as R
import refute_rows as rr

# witness -> the value from which the kernel's path is taken
PATH_REACHED = {
    "halvings": 1,
    "decisions past lane 63 by activity": 1,
    "first-UIP walk gap": 64,
    "collection walk gap": 64,
    "final walk gap": 64,
    "deepest level": 256,
    "opposite offers lost": 1,
}
assert tuple(PATH_REACHED) == R.PATHS


def rename(v):
    """Monotone, three of four ids missing, every id beyond lane 63's."""
    return 4 * v + 61


def renamed(clauses):
    return [[rename(l) if l > 0 else -rename(-l) for l in c] for c in clauses]


# the rows of cdcl_sound_rows.random_row() that are renamed: four SAT, four UNSAT
# (test_cdcl_sound_paths.py asserts the split and that every one decides by activity past lane 63)
RENAMED = (1, 5, 6, 13, 3, 11, 12, 15)

PHP6_SELECTORS = list(range(43, 50))
TRIAL_SELECTOR = 50


def php6_selector_row():
    """PHP(6), pigeon clause i carrying the negated selector 43 + i, under the seven: with all
    of them it is PHP(6), and without any one a pigeon stays out."""
    f = [list(c) for c in R.php(6)]
    for i, s in enumerate(PHP6_SELECTORS):
        f[i] = f[i] + [-s]
    return f, list(PHP6_SELECTORS)


def hard_trial_row():
    """The same beside a clause that refutes 50 under the seven selectors: query 0 ends ASSUMED
    by propagation alone, and the trial without 50 is PHP(6)'s search."""
    f, a = php6_selector_row()
    return f + [[-TRIAL_SELECTOR] + [-s for s in PHP6_SELECTORS]], a + [TRIAL_SELECTOR]


def uip_gap_row():
    """Deciding -1 implies 2 .. 73 in clause order and [-2, -73] is falsified: the walk from 73
    down to 2 passes 70 unmarked entries of the conflict's own level.  Learns [1]."""
    return [[1, 2]] + [[1, v] for v in range(3, 73)] + [[1, 73], [-2, -73]]


def uip_gap_to_the_decision_row():
    """Level 1 is -1 alone; deciding -2 implies 4 .. 74 and [1, 2, -74] is falsified.  The walk
    from 74 passes 70 unmarked entries and ends on the decision -2 itself, the first UIP, with
    the lower-level literal -1 right below it.  Learns [2, 1]."""
    return [[2, v] for v in range(4, 74)] + [[2, 74], [1, 2, -74]]


def low_gap_row():
    """Deciding -1 implies 4 .. 73; deciding -2 implies 3 and [1, 2, -3] is falsified.  The first
    UIP is the decision -2, and the only lower-level literal, -1, lies 70 unmarked entries of
    level 1 further down: the collection finds nothing in its first 64-entry step and reads the
    backjump level in its second.  Learns [2, 1]."""
    return [[1, v] for v in range(4, 74)] + [[2, 3], [1, 2, -3]]


def final_gap_row():
    """The assumption 1 implies 2 .. 72 and then, by [-2, -80], -80: the assumption 80 is false.
    The final analysis goes from -80 to 2, the lowest of the 71 entries implied, past the 70
    unmarked ones above it, and from 2 to the assumption 1.  ASSUMED, core [80, 1]."""
    return [[-1, 2]] + [[-1, v] for v in range(3, 73)] + [[-2, -80]], [1, 80]


def opposite_offers_row(apart, long_clause=False):
    """Deciding -1 makes [1, 2] and [1, -2] unit in one round, `apart` clauses from each other:
    2 stands, [1, -2] is falsified in the next round, and [1] is learned."""
    f = [[1, 2]] + [[1, v] for v in range(3, 2 + apart)] + [[1, -2]]
    return f + ([list(range(100, 112))] if long_clause else [])


RESUME_AT = 200


@functools.lru_cache(maxsize=None)
def rows():
    """(name, formula, assumptions, carry, conflict_limit) tuples."""
    php6 = R.php(6)
    rand = R.random_row()
    out = [
        ("php 6", php6, [], [], 0),
        ("two halvings", rr.random_3sat(6, 80, 340, 3)[0], [], [], 0),
        ("uip gap", uip_gap_row(), [], [], 0),
        ("uip gap to the decision", uip_gap_to_the_decision_row(), [], [], 0),
        ("low gap", low_gap_row(), [], [], 0),
        ("level 300", R.learned_length_row(300), [], [], 0),
        ("final gap",) + final_gap_row() + ([], 0),
        ("php 6 under selectors",) + php6_selector_row() + ([], 0),
        ("hard trial",) + hard_trial_row() + ([], 0),
        ("resumed: the first slice", php6, [], [], RESUME_AT),
        ("resumed", php6, [], C.solve(php6, (), RESUME_AT)["kept"], 0),
        ("opposite offers in one step", opposite_offers_row(1), [], [], 0),
        ("opposite offers 64 clauses apart", opposite_offers_row(64), [], [], 0),
        ("opposite offers beside a long clause", opposite_offers_row(64, True), [], [], 0),
    ]
    out += [(f"renamed {i}", renamed(rand[i]), [], [], 0) for i in RENAMED]
    return tuple(out)


def row(name):
    return next(r for r in rows() if r[0] == name)


# row -> the witnesses it must drive to PATH_REACHED (or to the value given)
NEEDS = {
    "php 6": {"halvings": 1},
    "two halvings": {"halvings": 2},
    "uip gap": {"first-UIP walk gap": 70},
    "uip gap to the decision": {"first-UIP walk gap": 70},
    "low gap": {"collection walk gap": 70},
    "level 300": {"deepest level": 300},
    "final gap": {"final walk gap": 70},
    "php 6 under selectors": {"halvings": 1},
    "hard trial": {"halvings": 1},
    "resumed": {},          # (no halving: that is the row; test_cdcl_sound_paths.py says why)
    "resumed: the first slice": {},
    "opposite offers in one step": {"opposite offers lost": 1},
    "opposite offers 64 clauses apart": {"opposite offers lost": 1},
    "opposite offers beside a long clause": {"opposite offers lost": 1},
}
NEEDS.update({f"renamed {i}": {"decisions past lane 63 by activity": 1} for i in RENAMED})
HALVING_ROWS = tuple(n for n, need in NEEDS.items() if "halvings" in need)
CHAIN_ROWS = ("php 6 under selectors", "hard trial")      # the rows of the shrinking kernel


@functools.lru_cache(maxsize=None)
def want(name, entry="carry", assumed=True):
    """The rule's result at a row (computed once, shared and never changed): by the sound, the
    assume, the carry or the shrink restatement; `assumed` False = without the row's assumptions."""
    _, f, a, carry, limit = row(name)
    a = a if assumed else []
    if entry == "sound":
        assert not a and not carry
        return R.solve(f, limit)
    if entry == "assume":
        assert not carry
        return A.solve(f, a, limit)
    if entry == "carry":
        return C.solve(f, a, limit, carry)
    assert entry == "shrink"
    return S.solve(f, a, limit, carry)


def paths_of(name):
    """The row's witnesses: over every query of the chain at a chain row."""
    if name in CHAIN_ROWS:
        qs = want(name, "shrink")["queries"]
        return {k: max(q["paths"][k] for q in qs) for k in R.PATHS}
    return want(name)["paths"]
