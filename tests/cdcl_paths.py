"""Formulas that drive the CDCL kernel (csrc/cdcl.hip) down each of its
structural paths, shared by tests/test_cdcl_paths.py (CPU: the oracle's path
counters prove every row reaches what it claims) and
tests/test_cdcl_paths_gpu.py (GPU: every row bit-exact against the oracle).

The counters are oracle.CDCL_PATHS (oracle/cdcl_oracle.c CDCL_P_*), stated in
the kernel's terms.  PATH_REACHED gives, per counter, the value from which the
kernel's path is taken; a row lists the counters it must drive there (or
further, where the row is about a boundary).

What the reference's search looks like, which shapes the rows: nothing is ever
propagated (its unit branch needs a watched clause of one literal, and watched
clauses have two or more), so every assigned variable above level 0 is a
decision on a level of its own; a conflict clause is learned as a copy of
itself, the search backtracks one decision, the bumped variable is decided
again and the same literals conflict again.  So

  * a formula has ONE conflicting literal list for its whole run, and every
    learned clause is a copy of it: a clause with repeats of <= 64 entries and
    one of > 64 entries cannot both be learned in one formula -- the two
    activity-bump forms have a row each (repeat_20x2 / repeat_40x2,
    repeat_33x2_1), and meet in one launch in the second-tenant batch;
  * activities are 0 or the same running sum of var_inc, once per occurrence
    in that list: two of them differ by a factor (m + 1) / m at least for
    occurrence counts m, so doubles that agree in the high word and differ in
    the low one (2^-20 relative) need a clause of about 2^20 entries.  No
    small formula reaches `decide_low_word`; it is asserted 0 over all rows
    instead of being required (PATHS_NEVER);
  * no variable above level 0 has an antecedent, so analyze_conflict never
    resolves (`resolve_steps`, `resolve_alen_max`) and never learns a unit
    clause (`learned_unit`): asserted 0 as well.
"""
import functools
import random

import oracle

# counter -> the value from which the kernel's path is taken
PATH_REACHED = {
    "false_key_index_max": 64,      # a false key in the second 64-key batch (k0 = 64)
    "stream_len_max": 257,          # a batch's stream longer than one 256-slot window
    "conflict_pos_max": 256,        # a conflict in a later window
    "conflict_later_chunk": 1,      # a conflict in chunk 1-3 of the first window
    "conflict_later_window": 1,
    "straddle_members": 1,          # a table that began in an earlier window (the prefix max's carry)
    "repl_pos_max": 3,              # a replacement watch found by the tail loop (CDCL_LITS_AHEAD = 3)
    "tail_skip_self": 1,            # the tail loop's `continue`
    "dup_visit_passes": 1,
    "conflict_len_max": 65,         # a conflict list of more than one 64-lane chunk
    "learned_len_max": 65,
    "maxlevel_pos_max": 64,         # the first maximal-level literal in a later chunk
    "learned_repeat_le64": 1,       # the lanes' activity bump with a repeated variable
    "learned_repeat_gt64": 1,       # the lane-0 bump with a repeated variable
    "learned_len_64": 1,            # the two sides of the bump forms' boundary
    "learned_len_65": 1,
    "table_slots_max": 8192,        # a table past WS_BITMAP_SLOTS = 4,096
    "resize_le_4096": 1,            # re-insertion against the register bitmap
    "resize_gt_4096": 1,            # re-insertion on lane 0
    "resize_used_gt_50000": 1,      # growth x2
    "add_dummy_reuse": 1,
    "add_multi_run": 1,             # a probe restarted with perturbation
    "add_single_slot": 1,           # i + 9 > mask
    "add_single_slot_big": 1,       # ... in a table that also has 10-slot runs
    "add_present": 1,
    "decide_tie": 1,                # equal maximal activities: the lowest index wins
}
# counters no formula of the reference's search moves (module docstring): 0 over every row
PATHS_NEVER = ("resolve_steps", "resolve_alen_max", "learned_unit", "decide_low_word")


def neg(L):
    """One all-negative clause [-1 .. -L]: L literals on L levels, every
    activity tied, the maximal-level literal last."""
    return [[-i for i in range(1, L + 1)]]


def neg_desc(L):
    """The same clause descending: the maximal-level literal first, two watch keys."""
    return [[-i for i in range(L, 0, -1)]]


def doubled(n, extra=0):
    """n negative literals, each twice in a row, then `extra` more single ones."""
    return [[-i for i in range(1, n + 1) for _ in range(2)] + [-i for i in range(n + 1, n + extra + 1)]]


def overlap():
    return [[-i for i in range(1, 71)], [-i for i in range(5, 80)]]


def binary(n):
    """n clauses [-i, -(i + n)]: 2n watch keys, false keys beyond the first 64."""
    return [[-i, -(i + n)] for i in range(1, n + 1)]


def windows():
    """40 clauses [-i, -(i + 40), -81]: 40 false keys of >= 8 slots, a stream of several windows."""
    return [[-i, -(i + 40), -81] for i in range(1, 41)]


def straddle(at):
    """20 small false tables (160 slots), then literal -21 watching 251 clauses in
    a 512-slot table that begins in the first window and ends in the third; the
    clause at index `at` is [-21, -1], the conflict once 1 and 21 are true."""
    f = [[-i, 100 + i] for i in range(1, 21)] + [[-21, 200 + j % 7] for j in range(250)]
    f.insert(at, [-21, -1])
    return f


def late():
    """Clauses of 5-9 literals watched by -3 whose literals before position 3
    are false when 1, 2, 3 are true and whose position 3 repeats -3 itself:
    the replacement (or none: the last clause) is found by the tail loop."""
    f = [[-3, -2, -1, -3] + [-3] * (t % 3) + [-2, -1][:t % 2 + 1] + [10 + t] for t in range(8)]
    return f + [[-3, -2, -1, -3, -2, -1, -3]]


def same_two(n):
    """n copies of [1, 2] and [-1, -2]: two tables of n members."""
    return [[1, 2]] * n + [[-1, -2]]


def few_watchers():
    """900 clauses watched by three literals (as test_cdcl_large_watch_tables'
    third formula): moves leave dummies, adds reuse them, collide along the
    probe runs and restart with perturbation."""
    rng = random.Random(8)
    f = []
    for _ in range(900):
        first = rng.choice((1, -1, 2))
        f.append([first] + [v if rng.random() < 0.5 else -v for v in rng.sample(range(3, 9), rng.randint(1, 3))])
    return f


GE, EQ = ">=", "=="

# (name, builder, max_iter, ((counter, GE | EQ, value), ...))
CDCL_PATH_ROWS = [
    ("neg_63", lambda: neg(63), 300, (("conflict_len_max", EQ, 63), ("learned_len_64", EQ, 0),
                                      ("conflict_later_window", GE, 1), ("dup_visit_passes", GE, 1),
                                      ("decide_tie", GE, 1), ("add_present", GE, 1))),
    ("neg_64", lambda: neg(64), 300, (("learned_len_64", GE, 100), ("learned_len_max", EQ, 64),
                                      ("maxlevel_pos_max", EQ, 63))),
    ("neg_65", lambda: neg(65), 300, (("learned_len_65", GE, 100), ("learned_len_max", EQ, 65),
                                      ("conflict_len_max", EQ, 65), ("maxlevel_pos_max", EQ, 64),
                                      ("false_key_index_max", GE, 64))),
    ("neg_70", lambda: neg(70), 300, (("maxlevel_pos_max", EQ, 69), ("repl_pos_max", GE, 64),
                                      ("tail_skip_self", GE, 1))),
    ("neg_130", lambda: neg(130), 300, (("conflict_len_max", EQ, 130), ("learned_len_max", EQ, 130),
                                        ("maxlevel_pos_max", EQ, 129), ("false_key_index_max", GE, 128),
                                        ("decide_tie", GE, 129))),
    ("neg_desc_70", lambda: neg_desc(70), 300, (("maxlevel_pos_max", EQ, 0), ("conflict_len_max", EQ, 70))),
    ("repeat_20x2", lambda: doubled(20), 300, (("learned_repeat_le64", GE, 100), ("learned_repeat_gt64", EQ, 0),
                                               ("conflict_later_chunk", GE, 1))),
    ("repeat_40x2", lambda: doubled(40), 300, (("learned_repeat_gt64", GE, 100), ("learned_len_max", EQ, 80))),
    ("repeat_33x2_1", lambda: doubled(33, 1), 300, (("learned_repeat_gt64", GE, 100), ("learned_len_max", EQ, 67))),
    ("overlap", overlap, 600, (("learned_len_max", EQ, 70), ("dup_visit_passes", GE, 100))),
    ("binary_100", lambda: binary(100), 400, (("false_key_index_max", GE, 128), ("add_single_slot_big", GE, 1))),
    ("windows", windows, 400, (("stream_len_max", GE, 320), ("conflict_later_chunk", GE, 1),
                               ("add_dummy_reuse", GE, 1), ("add_multi_run", GE, 1))),
    ("straddle_150", lambda: straddle(150), 300, (("straddle_members", GE, 50), ("conflict_later_window", GE, 1),
                                                  ("conflict_pos_max", GE, 256))),
    ("straddle_240", lambda: straddle(240), 300, (("straddle_members", GE, 100), ("conflict_pos_max", GE, 384))),
    ("late", late, 200, (("repl_pos_max", GE, 8), ("tail_skip_self", GE, 1), ("learned_repeat_le64", GE, 1))),
    ("resize_8192", lambda: same_two(3000), 6, (("table_slots_max", EQ, 8192), ("resize_le_4096", GE, 1),
                                                ("resize_gt_4096", GE, 2), ("resize_used_gt_50000", EQ, 0))),
    # the first resize with more than 50,000 members is the one out of 131,072
    # slots, at 78,643 of them.  Measured on the MI355X: 0.43 s for the LDS and
    # the arena run together (~160 k serial watch adds, lane-0 re-insertions), 0.05 s on the oracle
    ("growth_x2", lambda: same_two(78700), 6, (("resize_used_gt_50000", GE, 2), ("table_slots_max", EQ, 262144))),
    ("few_watchers", few_watchers, 300, (("add_dummy_reuse", GE, 1), ("add_multi_run", GE, 1),
                                         ("add_single_slot", GE, 1), ("add_single_slot_big", GE, 1),
                                         ("add_present", GE, 1), ("straddle_members", GE, 1))),
]

STAT_KEYS = ("iterations", "conflicts", "decisions", "learned", "clauses", "watch_keys", "level")


@functools.lru_cache(maxsize=None)
def row_formula(name):
    return next(r for r in CDCL_PATH_ROWS if r[0] == name)[1]()


@functools.lru_cache(maxsize=None)
def row_oracle(name):
    """The oracle's run of a row with its path counters, once per process."""
    row = next(r for r in CDCL_PATH_ROWS if r[0] == name)
    return oracle.cdcl(row_formula(name), row[2], paths=True)
