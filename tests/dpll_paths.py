"""Formulas that drive the general DPLL kernel (csrc/dpll.hip) down each of its
structural paths, shared by tests/test_dpll_paths.py (CPU: the oracle's path
counters prove every row reaches what it claims) and
tests/test_dpll_paths_gpu.py (GPU: every row bit-exact against the oracle, in
both storage forms of the kernel).

The counters are oracle.DPLL_PATHS (oracle/sat_oracle.c DP_*), stated in the
kernel's terms.  PATH_REACHED gives, per counter, the value from which the
kernel's path is taken; a row lists the counters it must drive there (or
further, where the row is about a boundary).

Structural facts of the reference's search, which shape the rows:

  * A unit can contradict the assignment (REF.py:150, the kernel's `mis`) only
    where the assignment did not reduce the formula: an effective assignment of
    l drops every clause with l and shortens every clause with -l, so a later
    unit [-l] is an emptied clause, found when l is assigned, not a mismatch.
    The assignments that do not reduce the formula are the caller's dict and a
    REF-mode decision.  A REF-mode decision is followed by no propagation that
    could meet it (nothing becomes unit when the formula does not change), so
    the rows for the mismatch counters use a caller's dict; `decision_mismatch`
    is asserted 0 over all rows instead of being required (PATHS_NEVER).
  * For the same reason a REF-mode search propagates at its root only, never
    finds new pure literals below a decision, and each of its backtracks undoes
    exactly the decision: `undo_len_max` past 64 is a SOUND-mode row.
  * `snapshot_same_var_opposite_sign` counts what the kernel sees: [l] and [-l]
    in one 64-entry chunk, where the loser's clause is emptied at the winner's
    time stamp.  With [-l] in a later chunk the kernel stops before reaching it
    (row opposite_sign_later_chunk: the cut then undoes the rest of chunk 0).
  * `model_mismatch` counts events that contradict the oracle's account of what
    the kernel runs (which of the reference's snapshot entries the kernel's
    snapshot holds, where it stops): 0 over all rows.
"""
import functools
import random

import oracle

# counter -> the value from which the kernel's path is taken
PATH_REACHED = {
    "snapshot_len_max": 65,                 # the second k0 chunk of propagate
    "collected_snapshot_len_max": 65,       # ... of a snapshot made by collect_units
    "stamp_drop_len_max": 65,               # nu > 64: time stamps dropped along the trail
    "mismatch_index_max": 64,               # kmis in a later chunk
    "emptied_index_max": 64,                # e_min in a later chunk
    "undone_after_stop_max": 1,             # apply_trail<UNDO>(cut, trail_len) has work
    "cut_round_len_max": 65,                # the `keep` scan over more than one wave step
    "snapshot_same_var_same_sign": 1,
    "snapshot_same_var_opposite_sign": 1,
    "snapshot_same_var_earlier_chunk": 1,
    "skip_assigned_equal": 1,
    "empty_clause_with_units": 1,
    "empty_clause_no_units": 1,
    "empty_clause_first_index_max": 64,     # first_k kept across chunks
    "occ_single_len_max": 65,               # the single-literal form past one wave step
    "flat_total_max": 65,                   # the flattened form past one 64-slot window
    "flat_list_straddles_window": 1,        # the `carry` owner
    "unit_clause_index_max": 4096,          # the second w0 pass of collect_units
    "conflict_clauses_max": 4097,           # ... of clear_ubits
    "pure_count_max": 65,                   # apply_trail over more than 64 pure literals
    "pure_first_pos_max": 4096,             # the second w0 pass of assign_pures
    "branch_var_max": 65,                   # the second v0 group of analyze
    "branch_tie_across_groups": 1,
    "undo_len_max": 65,                     # unassign_to over more than one wave step
    "undo_non_effective": 1,
    "init_overwrite": 1,
    "init_var_beyond_formula": 1,
    "init_mismatch": 1,
    "sols_past_cap": 1,
    "clause_len_max": 256,                  # past Narrow::MAX_LEN: the wide form only
}
# counters no formula moves (module docstring): 0 over every row
PATHS_NEVER = ("decision_mismatch", "model_mismatch")

NARROW_MAX_LEN = 255     # csrc/dpll.hip Narrow::MAX_LEN
LDS_LIMIT = 160 * 1024   # make_layout's bound: one workgroup's LDS


def lds_bytes(max_vars, max_clauses, max_lits):
    """make_layout (csrc/dpll.hip) restated: the bytes of one wave's LDS image
    (satmi_dpll_lds_bytes, which test_dpll_paths.py compares it with); 0 when the
    16-bit fields do not hold the shape."""
    if max_vars > 32766 or max_clauses > 65534 or max_lits > 65535:
        return 0
    N, M, Lc = max_vars + 1, max_clauses + 1, max_lits + 1

    def a16(x):
        return (x + 15) & ~15
    o = 0
    for size in (2 * (Lc + 4), 2 * M, 2 * (2 * N + 1), 2 * Lc, 4 * M, 4 * N, 4 * N, 4 * N, 2 * N, 2 * N, 2 * N,
                 2 * M, 8 * ((M + 63) // 64), 8 * ((Lc + 63) // 64), 4 * 64):
        o = a16(o + size)
    return o


def narrow_shape(bytes_per_wave):
    """narrow_shape (csrc/dpll.hip) restated: (waves per workgroup, waves per CU)."""
    best = (1, 0)
    for wpg in (4, 2, 1):
        wgs = min(16, LDS_LIMIT // (bytes_per_wave * wpg))
        waves = min(32, wgs * wpg)
        if wgs >= 1 and waves > best[1]:
            best = (wpg, waves)
    return best


def shape_of(formula, init=()):
    """(max_vars, max_clauses, max_lits, max_clause_len) of a one-instance batch."""
    nv = max([abs(l) for c in formula for l in c] + [abs(l) for l in init] + [0])
    return nv, len(formula), sum(len(c) for c in formula), max([len(c) for c in formula] + [0])


def units(n):
    return [[i] for i in range(1, n + 1)]


def units_with(at, clause, n=200):
    """n unit clauses [1] .. [n] with `clause` inserted at index `at`."""
    f = units(n)
    f.insert(at, clause)
    return f


def fanout_propagated():
    return [[1]] + [[-1, i] for i in range(2, 152)]


def fanout_decision():
    return ([[-1, i] for i in range(2, 152)] +
            [[-70, -90], [1, 200], [1, -200], [1, 201], [-1, 201, 202]])


def hub(n=100):
    """No pure literal; variable 1 occurs most.  SOUND: 1 = True makes n clauses
    unit at once, [-70, -90] conflicts, the backtrack undoes n + 1 trail entries."""
    return ([[-1, i] for i in range(2, n + 2)] + [[1, -i] for i in range(2, n + 2)] + [[-70, -90]])


def pures(pad_lits=0):
    """199 clauses [i, i + 1000]: 398 pure literals; `pad_lits` literals of
    clauses over two variables that are never pure in front of them."""
    pad = []
    while pad_lits >= 4:
        pad += [[2000, -2001], [-2000, 2001]]
        pad_lits -= 4
    assert pad_lits == 0
    return pad + [[i, i + 1000] for i in range(1, 200)]


def pure_at(pos):
    """A pure variable whose first occurrence is literal `pos` of the formula."""
    assert pos % 4 in (0, 3)
    pad = [[2, -3], [-2, 3]] * (pos // 4) + ([[2, -3, -2]] if pos % 4 else [])
    assert sum(len(c) for c in pad) == pos
    return pad + [[7, 7]]


def unit_at(index):
    """Clause `index` is [-1, 5], unit once [1] (clause 0) is propagated."""
    return [[1]] + [[2, 3]] * (index - 1) + [[-1, 5]]


def random_3cnf(n, m, seed):
    rng = random.Random(seed)
    f = [[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), 3)] for _ in range(m)]
    f[0][0] = n
    return f


def many_clauses():
    """4,200 random 3-literal clauses over 300 variables, then a chain hanging off
    variable 1 in clauses of index >= 4,200: they turn unit by propagation."""
    f = random_3cnf(300, 4200, 5)
    return f + [[-1, 301], [1, 302]] + [[-301, 303], [-302, 304], [-303, -304, 305]]


def long_clause(Lc, empty=False, dups=False):
    c = list(range(1, Lc + 1))
    if dups:   # a repeated literal and a tautology inside the long clause, its length kept
        c[10], c[20] = 5, -7
    return ([[]] if empty else []) + [c, [-1, -2], [2, -3]]


def empty_with_units(n=70, extra=()):
    return [[]] + units(n) + [list(c) for c in extra]


def shape_row(n, m, seed):
    return random_3cnf(n, m, seed)


# One-instance shapes of random 3-literal clauses by their LDS image (lds_bytes):
# (variables, clauses) -> the workgroup class narrow_shape takes, or the wide form.
SHAPE_ROWS = {
    "shape_4_waves": (40, 170),         # 4.7 KiB: 4 waves per workgroup, 32 per CU
    "shape_2_waves": (400, 2500),       # 53.4-80 KiB: 2 waves per workgroup, > 64 KiB per workgroup
    "shape_1_wave": (800, 5000),        # 80-160 KiB: 1 wave per workgroup, > 64 KiB
    "shape_under_160k": (900, 7007),    # exactly 160 KiB: the last shape of the LDS form
    "shape_over_160k": (900, 7008),     # 64 bytes more: AUTO takes the wide form
}
SHAPE_CLASS = {"shape_4_waves": 4, "shape_2_waves": 2, "shape_1_wave": 1, "shape_under_160k": 1,
               "shape_over_160k": 0}

GE, EQ = ">=", "=="
SOUND, REF = "sound", "ref"


def kw(mode=SOUND, node_limit=400, sol_cap=8, init=None):
    return {"mode": mode, "node_limit": node_limit, "sol_cap": sol_cap, "init": init}


# (name, builder, kwargs of oracle.dpll under which `needs` hold, ((counter, GE | EQ, value), ...))
DPLL_PATH_ROWS = [
    # ---- root snapshots around the 64-entry chunk edges
    ("units_64", lambda: units(64), kw(), (("snapshot_len_max", EQ, 64), ("stamp_drop_len_max", EQ, 64))),
    ("units_65", lambda: units(65), kw(), (("snapshot_len_max", EQ, 65), ("stamp_drop_len_max", EQ, 65))),
    ("units_128", lambda: units(128), kw(), (("snapshot_len_max", EQ, 128), ("stamp_drop_len_max", EQ, 128))),
    ("units_129", lambda: units(129), kw(), (("snapshot_len_max", EQ, 129), ("stamp_drop_len_max", EQ, 129))),
    ("units_200", lambda: units(200), kw(), (("snapshot_len_max", EQ, 200), ("stamp_drop_len_max", EQ, 200))),
    # ---- a clause emptied by unit k: the cut, the undo of the chunk's rest
    ("emptied_63", lambda: units(200) + [[-30, -64]], kw(), (("emptied_index_max", EQ, 63),
                                                             ("undone_after_stop_max", EQ, 0))),
    ("emptied_64", lambda: units(200) + [[-30, -65]], kw(), (("emptied_index_max", EQ, 64),
                                                             ("undone_after_stop_max", EQ, 63),
                                                             ("cut_round_len_max", EQ, 128))),
    ("emptied_69", lambda: units(200) + [[-30, -70]], kw(), (("emptied_index_max", EQ, 69),
                                                             ("undone_after_stop_max", EQ, 58))),
    ("emptied_129", lambda: units(200) + [[-100, -130]], kw(), (("emptied_index_max", EQ, 129),
                                                                ("undone_after_stop_max", EQ, 62),
                                                                ("cut_round_len_max", EQ, 192),
                                                                ("conflict_clauses_max", EQ, 201))),
    # ---- one variable twice in a snapshot
    ("opposite_sign_same_chunk", lambda: units_with(40, [-3]), kw(),
     (("snapshot_same_var_opposite_sign", GE, 1), ("emptied_index_max", EQ, 2), ("undone_after_stop_max", EQ, 60))),
    ("opposite_sign_later_chunk", lambda: units_with(149, [-3]), kw(),
     (("emptied_index_max", EQ, 2), ("undone_after_stop_max", EQ, 61), ("snapshot_len_max", EQ, 201))),
    ("same_sign", lambda: units_with(150, [9], 199)[:30] + [[5]] + units_with(150, [9], 199)[30:], kw(),
     (("snapshot_same_var_same_sign", EQ, 1), ("snapshot_same_var_earlier_chunk", EQ, 1),
      ("snapshot_len_max", EQ, 201))),
    # ---- a unit against the caller's dict
    ("mismatch_149_sound", lambda: units_with(149, [-3]), kw(init=[3]),
     (("mismatch_index_max", EQ, 149), ("init_mismatch", GE, 1), ("skip_assigned_equal", GE, 1))),
    ("mismatch_2_ref", lambda: units_with(149, [-3]), kw(REF, init=[-3]),
     (("mismatch_index_max", EQ, 2), ("init_mismatch", GE, 1))),
    ("mismatch_63", lambda: units(200), kw(init=[-64]), (("mismatch_index_max", EQ, 63),)),
    ("mismatch_64", lambda: units(200), kw(REF, init=[-65]), (("mismatch_index_max", EQ, 64),
                                                              ("conflict_clauses_max", EQ, 200))),
    # ---- the caller's dict itself
    ("init_overwrite", lambda: units(70) + [[71, 72], [-71, 72]], kw(REF, init=[3, 500, -3, 71, 3]),
     (("init_overwrite", EQ, 2), ("init_var_beyond_formula", EQ, 1), ("skip_assigned_equal", GE, 1))),
    ("init_overwrite_mismatch", lambda: units(70), kw(init=[3, 40, -3]),
     (("init_overwrite", EQ, 1), ("init_mismatch", GE, 1), ("mismatch_index_max", EQ, 2))),
    # ---- occurrence lists past one wave step
    ("fanout_propagated", fanout_propagated, kw(),
     (("occ_single_len_max", GE, 151), ("collected_snapshot_len_max", EQ, 150), ("flat_total_max", GE, 64))),
    ("fanout_decision_sound", fanout_decision, kw(),
     (("pure_count_max", EQ, 150), ("occ_single_len_max", GE, 150), ("flat_total_max", GE, 150),
      ("flat_list_straddles_window", GE, 1))),
    ("fanout_decision_ref", fanout_decision, kw(REF),
     (("sols_past_cap", EQ, 8), ("branch_var_max", GE, 200), ("branch_tie_across_groups", GE, 1),
      ("undo_non_effective", GE, 1), ("pure_count_max", EQ, 150))),
    ("hub_64", lambda: hub(63), kw(), (("undo_len_max", EQ, 64), ("collected_snapshot_len_max", EQ, 63))),
    ("hub_65", lambda: hub(64), kw(), (("undo_len_max", EQ, 65), ("collected_snapshot_len_max", EQ, 64))),
    ("hub_101", lambda: hub(100), kw(), (("undo_len_max", EQ, 101), ("collected_snapshot_len_max", EQ, 100),
                                        ("occ_single_len_max", GE, 200))),
    # ---- pure literals
    ("pures_398", pures, kw(), (("pure_count_max", EQ, 398),)),
    ("pures_padded", lambda: pures(4100), kw(), (("pure_count_max", EQ, 398), ("pure_first_pos_max", GE, 4097))),
    ("pure_at_4095", lambda: pure_at(4095), kw(), (("pure_first_pos_max", EQ, 4095),)),
    ("pure_at_4096", lambda: pure_at(4096), kw(), (("pure_first_pos_max", EQ, 4096),)),
    # ---- more than 4,096 clauses
    ("unit_at_4095", lambda: unit_at(4095), kw(), (("unit_clause_index_max", EQ, 4095),)),
    ("unit_at_4096", lambda: unit_at(4096), kw(), (("unit_clause_index_max", EQ, 4096),)),
    ("many_clauses", many_clauses, kw(),
     (("unit_clause_index_max", GE, 4096), ("conflict_clauses_max", GE, 4097), ("undo_len_max", GE, 2),
      ("flat_list_straddles_window", GE, 1), ("branch_tie_across_groups", GE, 1))),
    # ---- the empty clause
    ("empty_alone", lambda: [[]], kw(), (("empty_clause_no_units", GE, 1),)),
    ("empty_with_70_units", empty_with_units, kw(),
     (("empty_clause_with_units", GE, 1), ("empty_clause_first_index_max", EQ, 0), ("undone_after_stop_max", EQ, 63))),
    ("empty_first_63", empty_with_units, kw(init=list(range(1, 64))),
     (("empty_clause_first_index_max", EQ, 63), ("skip_assigned_equal", GE, 63))),
    ("empty_first_64", empty_with_units, kw(init=list(range(1, 65))),
     (("empty_clause_first_index_max", EQ, 64), ("undone_after_stop_max", EQ, 5))),
    ("empty_then_decision", lambda: [[]] + [[1, 2], [-1, 2], [1, -2]], kw(),
     (("empty_clause_no_units", GE, 1), ("empty_clause_with_units", GE, 1))),
    # ---- duplicate literals and tautologies
    ("dups_in_snapshot", lambda: units_with(10, [4, 4]) + [[6, -6], [-8, -8, 201], [201, -201, -9]], kw(),
     (("snapshot_len_max", EQ, 200), ("collected_snapshot_len_max", GE, 1))),
    # ---- clause length around Narrow::MAX_LEN
    ("long_255", lambda: long_clause(255), kw(), (("clause_len_max", EQ, 255), ("pure_count_max", GE, 252))),
    ("long_256", lambda: long_clause(256), kw(), (("clause_len_max", EQ, 256), ("pure_count_max", GE, 253))),
    ("long_300", lambda: long_clause(300), kw(), (("clause_len_max", EQ, 300), ("pure_count_max", GE, 297))),
    ("long_300_empty", lambda: long_clause(300, empty=True), kw(),
     (("clause_len_max", EQ, 300), ("empty_clause_no_units", GE, 1))),
    ("long_300_dups", lambda: long_clause(300, dups=True), kw(), (("clause_len_max", EQ, 300),)),
] + [
    # ---- LDS shape classes (test_dpll_paths.py proves each shape's class)
    (name, functools.partial(shape_row, n, m, 40 + i), kw(node_limit=60), (("clause_len_max", EQ, 3),))
    for i, (name, (n, m)) in enumerate(SHAPE_ROWS.items())
]

LONG_ROWS = tuple(name for name, _, _, needs in DPLL_PATH_ROWS
                  if any(c == "clause_len_max" and v > NARROW_MAX_LEN for c, _, v in needs))

CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")


def row(name):
    return next(r for r in DPLL_PATH_ROWS if r[0] == name)


@functools.lru_cache(maxsize=None)
def row_formula(name):
    return row(name)[1]()


@functools.lru_cache(maxsize=None)
def row_oracle(name, mode=None):
    """The oracle's run of a row (in the row's own mode, or `mode`) with its path
    counters, once per process."""
    k = dict(row(name)[2])
    if mode is not None:
        k["mode"] = mode
    return oracle.dpll(row_formula(name), max_solutions=0, paths=True, **k)
