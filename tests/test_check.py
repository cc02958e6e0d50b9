"""CPU checks of the batched model check (csrc/check.hip, satmi/check.py).

The expected values of tests/test_check_gpu.py come from check_rows.evaluate;
here that evaluator is first held to brute force and to the hand-built rows.
satmi_check_models_host validates its arguments before any HIP call, so every
return below comes back without a GPU."""
import ctypes
import itertools
import json
import os
import random

import numpy as np
import pytest

import check_rows as cr
from satmi import _capi
from satmi.check import check_models, check_packed, debug_grid
from satmi.cnf import pack

ERR_ARG, ERR_TOO_LARGE = -1, -3


# ------------------------------------------------------------------ the evaluator
def test_evaluator_matches_brute_force():
    """On formulas of at most 6 variables, over ALL total assignments: ok == every clause
    has a true literal; a total assignment leaves nothing undetermined, and the first
    falsified index is the first clause without a true literal."""
    rng = random.Random(11)
    formulas = [[], [[]], [[1], []], [[1, -1]], [[1, 1, -2]]]
    for _ in range(60):
        n = rng.randint(1, 6)
        formulas.append([[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), rng.randint(1, n))]
                         for _ in range(rng.randint(1, 12))])
    for f in formulas:
        n = cr.max_vars_of(f)
        for bits in itertools.product((False, True), repeat=n):
            row = [v if bits[v - 1] else -v for v in range(1, n + 1)]
            unsat = [i for i, c in enumerate(f) if not any(bits[abs(l) - 1] == (l > 0) for l in c)]
            w = cr.evaluate(f, row)
            assert w == [len(unsat), 0, unsat[0] if unsat else -1, 0], (f, row)
            assert cr.is_ok(w) == (not unsat)


def test_evaluator_on_the_hand_built_rows():
    # worked by hand from the rule, in EDGE_CASES' order
    want = [[0, 0, -1, 0], [0, 0, -1, 0], [2, 0, 1, 0], [0, 2, -1, 0], [1, 0, 2, 0], [0, 1, -1, 0], [0, 1, -1, 0],
            [0, 0, -1, 0], [1, 0, 0, 0], [1, 0, 1, 0], [1, 0, 2, 1], [1, 0, 1, 2], [0, 0, -1, 2], [1, 0, 1, 2],
            [0, 1, -1, 3]]
    got = [cr.evaluate(f, r, cr.EDGE_MAX_VARS) for f, r in cr.EDGE_CASES]
    assert got == want
    for k in cr.CLAUSE_LENGTHS:
        f, row = cr.length_case(k)
        assert [len(c) for c in f] == [k] * 3 and cr.evaluate(f, row) == [1, 1, 1, 0]
    for f, row, w in cr.count_cases():
        assert cr.evaluate(f, row) == w
    assert {len(f) for f, _, _ in cr.count_cases()} == set(cr.CLAUSE_COUNTS)
    f, rows = cr.reuse_disjoint(8)
    assert [cr.evaluate(f, r) for r in rows] == [[1, 14, 2 * k, 0] for k in range(8)]
    f, rows = cr.reuse_alternating(8)
    assert [cr.evaluate(f, r) for r in rows] == [[2, 0, 1 - k % 2, 0] for k in range(8)]


def test_reference_fixture_split(golden_dir):
    """The split of tests/golden/dpll_ref.json the GPU test pins: 107 of its 5,080 recorded
    solutions are models, 4,973 in 31 of its 105 cases are not (the reference never
    applies a branch to the formula)."""
    with open(os.path.join(golden_dir, "dpll_ref.json")) as fh:
        cases = json.load(fh)["cases"]
    oks = [[cr.is_ok(cr.evaluate(c["formula"], s)) for s in c["solutions"]] for c in cases]
    assert (sum(map(sum, oks)), sum(len(o) - sum(o) for o in oks)) == (107, 4973)
    assert (sum(1 for o in oks if not all(o)), len(cases)) == (31, 105)


# ------------------------------------------------------------------ the host form's argument checks
def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _call(formulas, rows_of, num=None, cap=None, stride=None, null=(), lits=None, nrows=None, lens=None):
    """satmi_check_models_host on `formulas` and their rows (formula literals overridden by
    `lits`, row counts by `nrows`, row lengths by `lens`), the arguments named in `null`
    passed as NULL -> (return code, message)."""
    L = _capi.load()
    icb = np.cumsum([0] + [len(f) for f in formulas]).astype(np.int32)
    clb = np.cumsum([0] + [len(c) for f in formulas for c in f]).astype(np.int32)
    flat = [l for f in formulas for c in f for l in c] if lits is None else lits
    la = np.array(flat or [0], dtype=np.int64).astype(np.int32)
    B = len(formulas)
    kcap = max([len(r) for r in rows_of] + [1])
    kstride = max([len(x) for r in rows_of for x in r] + [1])
    rows = np.array([len(r) for r in rows_of] if nrows is None else nrows, dtype=np.int32)
    ln = np.zeros((max(B, 1), kcap), dtype=np.int32)
    rl = np.zeros((max(B, 1), kcap, kstride), dtype=np.int32)
    for b, r in enumerate(rows_of):
        for k, x in enumerate(r):
            ln[b, k] = len(x)
            rl[b, k, :len(x)] = x
    if lens is not None:
        ln[:] = lens
    out = np.full((max(B, 1), kcap, 4), 7, dtype=np.int32)
    a = {"icb": _p(icb), "clb": _p(clb), "lits": _p(la), "rows": _p(rows), "len": _p(ln), "row_lits": _p(rl),
         "out": _p(out)}
    for k in null:
        a[k] = None
    rc = L.satmi_check_models_host(B if num is None else num, a["icb"], a["clb"], a["lits"], a["rows"], a["len"],
                                   a["row_lits"], kcap if cap is None else cap,
                                   kstride if stride is None else stride, a["out"])
    return rc, (L.satmi_last_error() or b"").decode()


F = [[[1, 2], [-1]], [[3]]]
R = [[[1, 2]], [[-3], [3]]]


def test_negative_count():
    rc, msg = _call(F, R, num=-1)
    assert rc == ERR_ARG and "satmi_check_models_host" in msg and "negative" in msg


@pytest.mark.parametrize("kw", [{"cap": 0}, {"cap": -1}, {"stride": 0}, {"stride": -5}])
def test_cap_and_stride_below_one(kw):
    rc, msg = _call(F, R, **kw)
    assert rc == ERR_ARG and next(iter(kw)) in msg


@pytest.mark.parametrize("name", ["icb", "clb", "lits", "len", "row_lits", "out"])
def test_null_required_pointer(name):
    rc, msg = _call(F, R, null=(name,))
    assert rc == ERR_ARG and "null" in msg


def test_non_ascending_ranges():
    L = _capi.load()
    one = np.zeros(4, dtype=np.int32)
    for icb, clb, word in (([0, 2, 1], [0, 1, 2], "clause ranges"), ([-1, 1, 2], [0, 1, 2], "clause ranges"),
                           ([0, 1, 2], [0, 2, 1], "literal ranges"), ([0, 1, 2], [-1, 0, 1], "literal ranges")):
        rc = L.satmi_check_models_host(2, _p(np.array(icb, dtype=np.int32)), _p(np.array(clb, dtype=np.int32)),
                                       _p(np.ones(4, dtype=np.int32)), None, _p(one), _p(one), 1, 1,
                                       _p(np.zeros(8, dtype=np.int32)))
        assert rc == ERR_ARG and word in L.satmi_last_error().decode()


@pytest.mark.parametrize("bad", [0, cr.I32_MIN])
def test_bad_formula_literal(bad):
    rc, msg = _call(F, R, lits=[1, 2, bad, 3])
    assert rc == ERR_ARG and "literal" in msg


def test_row_count_and_length_out_of_range():
    for nrows in ([1, 3], [-1, 2]):
        rc, msg = _call(F, R, nrows=nrows)
        assert rc == ERR_ARG and "row count" in msg
    for lens in (2, -1):
        rc, msg = _call(F, R, lens=lens, stride=1)
        assert rc == ERR_ARG and "row length" in msg


def test_max_vars_past_the_limit_is_too_large():
    """The limit of include/satmi.h, before any HIP call: in the formula or in a row."""
    assert _capi.CHECK_MAX_VARS == cr.MAX_VARS
    big = cr.MAX_VARS + 1
    rc, msg = _call([[[1, -big]]], [[[1]]])
    assert rc == ERR_TOO_LARGE and str(big) in msg
    rc, msg = _call([[[1, 2]]], [[[1, big]]])
    assert rc == ERR_TOO_LARGE and str(big) in msg
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        check_models([[[1, -big]]], [[[1]]])


def test_device_form_argument_errors():
    """satmi_check_models_device refuses what it can see before it touches the device."""
    L = _capi.load()
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below fails on its arguments
    for B, mv, mcl, cap, stride, rc in ((-1, 3, 3, 1, 1, ERR_ARG), (1, 3, 3, 0, 1, ERR_ARG), (1, 3, 3, 1, 0, ERR_ARG),
                                        (1, -1, 3, 1, 1, ERR_ARG), (1, 3, -1, 1, 1, ERR_ARG),
                                        (1, cr.MAX_VARS + 1, 3, 1, 1, ERR_TOO_LARGE), (0, 3, 3, 1, 1, _capi.OK)):
        assert L.satmi_check_models_device(B, p, p, p, mv, mcl, None, p, p, cap, stride, p, None) == rc
    assert L.satmi_check_models_device(1, p, p, p, 3, 3, None, None, p, 1, 1, p, None) == ERR_ARG
    assert "null" in L.satmi_last_error().decode()


def test_empty_batch_is_ok():
    assert _call([], [])[0] == _capi.OK
    assert _call([], [], null=("icb", "clb", "lits", "rows", "len", "row_lits", "out"))[0] == _capi.OK
    assert check_models([], []) == []
    assert check_packed(pack([]), None, np.zeros((0, 2), np.int32), np.zeros((0, 2, 3), np.int32)).shape == (0, 2, 4)


def test_wrapper_shapes_are_checked():
    with pytest.raises(ValueError):
        check_models([[[1]]], [])
    with pytest.raises(ValueError):
        check_packed(pack([[[1]]]), None, np.zeros((2, 1), np.int32), np.zeros((2, 1, 1), np.int32))


def test_debug_knob_arguments():
    try:
        debug_grid(1, 1)
        debug_grid(3, 4)
        for wgs, wpg in ((-1, 0), (0, 3), (0, 8), (0, -1)):
            with pytest.raises(_capi.SatmiError):
                debug_grid(wgs, wpg)
    finally:
        debug_grid(0, 0)
