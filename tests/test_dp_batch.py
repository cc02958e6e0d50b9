"""CPU checks of the batched Davis-Putnam entry point (csrc/dp_batch.hip): the
exports, the slot rule that orders the variables without set images, the
argument checks (all made before any HIP call, so every return below comes
back without a GPU), and the proofs that every hand-built row of
tests/test_dp_batch_gpu.py has the sizes, the variable order and the collision
step it claims -- derived from the oracle's record."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import dp_batch_rows as R
import oracle
from satmi import _capi, cnf
from satmi.dp import debug_batch, eliminate_batch, order_free_pop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NEW = ("satmi_dp_batch_host", "satmi_dp_debug_batch")


def _p(a, t=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(t))


# ---------------------------------------------------------------- exports
def test_exports():
    text = open(os.path.join(ROOT, "include", "satmi.h")).read()
    declared = set(re.findall(r"\b(satmi_[a-z0-9_]+)\s*\(", text))
    L = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTED and hasattr(L, name), name
    assert "#define SATMI_DP_BATCH_UNFIT (-2)" in text and _capi.DP_BATCH_UNFIT == -2
    assert L.satmi_abi_version() == 2


# ---------------------------------------------------------------- the slot rule
def _slots(n):
    return 8 if n <= 4 else 32 if n <= 18 else 128 if n <= 76 else None


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 17, 18, 19, 20, 25])
def test_pop_rule_matches_the_set_model(n):
    rng = random.Random(1000 + n)
    mask = _slots(n) - 1
    done = 0
    while done < 60:
        ids = rng.sample(range(1, 200), n)
        if len({v & mask for v in ids}) != n:
            assert order_free_pop(ids) is None
            continue
        done += 1
        want = order_free_pop(ids)
        assert want == min(ids, key=lambda v: v & mask)
        for order in (sorted(ids), sorted(ids, reverse=True), rng.sample(ids, n)):
            assert order_free_pop(order) == want
            assert oracle.pyset_var_pop([[v] for v in order]) == want, order
        # ... and as the variable set of clauses (two ids a clause, both signs)
        sh = rng.sample(ids, n)
        assert oracle.pyset_var_pop([[a, -b] for a, b in zip(sh, sh[1:] + sh[:1])]) == want


def test_pop_rule_named_cases():
    assert order_free_pop({3, 4, 5, 9}) == 9
    assert order_free_pop({15, 16}) == 16
    assert order_free_pop({3, 11}) is None
    assert order_free_pop([7]) == 7 and order_free_pop([]) is None
    # the table grows with the count alone: 8 -> 32 at five ids, 32 -> 128 at nineteen
    assert order_free_pop([1, 2, 3, 9]) is None and order_free_pop([1, 2, 3, 4, 9]) == 1
    assert order_free_pop(list(range(30, 48))) == 32 and order_free_pop(list(range(30, 49))) == 30
    # the insertion order decides exactly when two homes collide
    assert {oracle.pyset_var_pop([[3], [11]]), oracle.pyset_var_pop([[11], [3]])} == {3, 11}


def test_pop_rule_none_iff_homes_collide():
    rng = random.Random(5)
    seen = set()
    for _ in range(2000):
        n = rng.randint(1, 25)
        ids = rng.sample(range(1, 200), n)
        coll = len({v & (_slots(n) - 1) for v in ids}) != n
        assert (order_free_pop(ids) is None) == coll
        seen.add(coll)
    assert seen == {True, False}


# ---------------------------------------------------------------- argument checks
def _call(formulas, num=None, step_cap=4, null=(), lits=None, rec=()):
    """satmi_dp_batch_host on `formulas` (literals overridden by `lits`), the
    arguments named in `null` passed as NULL, the record pointers named in `rec`
    given -> (return code, message)."""
    L = _capi.load()
    icb = np.cumsum([0] + [len(f) for f in formulas]).astype(np.int32)
    clb = np.cumsum([0] + [len(c) for f in formulas for c in f]).astype(np.int32)
    flat = [l for f in formulas for c in f for l in c] if lits is None else lits
    la = np.array(flat or [0], dtype=np.int64).astype(np.int32)
    B = len(formulas) if num is None else num
    n = max(B, 1) * max(step_cap, 1)
    res, steps = np.full(max(B, 1), 7, np.int32), np.full(max(B, 1), 7, np.int32)
    tr, sc = np.zeros(n, np.int32), np.zeros(n, np.int64)
    rl, rco, rso = np.zeros(64, np.int32), np.zeros(64, np.int64), np.zeros(max(B, 1) * (max(step_cap, 0) + 1), np.int64)
    a = {"icb": _p(icb), "clb": _p(clb), "lits": _p(la), "res": _p(res), "steps": _p(steps), "tr": _p(tr),
         "sc": _p(sc, ctypes.c_int64)}
    for k in null:
        a[k] = None
    r = {"rl": _p(rl) if "rl" in rec else None, "rco": _p(rco, ctypes.c_int64) if "rco" in rec else None,
         "rso": _p(rso, ctypes.c_int64) if "rso" in rec else None}
    rc = L.satmi_dp_batch_host(B, a["icb"], a["clb"], a["lits"], 0, 0, a["res"], a["steps"], a["tr"], a["sc"],
                               step_cap, r["rl"], 64, r["rco"], 64, r["rso"])
    return rc, (L.satmi_last_error() or b"").decode()


F = [[[1, 2], [-1]], [[3]]]


def test_negative_count():
    rc, msg = _call(F, num=-1)
    assert rc == ERR_ARG and "satmi_dp_batch_host" in msg


def test_negative_step_cap():
    rc, msg = _call(F, step_cap=-1)
    assert rc == ERR_ARG and "step_cap" in msg


@pytest.mark.parametrize("name", ["icb", "clb", "lits", "res", "steps", "tr", "sc"])
def test_null_required_pointer(name):
    rc, msg = _call(F, null=(name,))
    assert rc == ERR_ARG and "null" in msg


@pytest.mark.parametrize("rec", [("rl",), ("rco",), ("rso",), ("rl", "rco"), ("rl", "rso"), ("rco", "rso")])
def test_partial_record_pointers(rec):
    rc, msg = _call(F, rec=rec)
    assert rc == ERR_ARG and "record" in msg


@pytest.mark.parametrize("bad", [0, -(2 ** 31)])
def test_bad_literal(bad):
    rc, msg = _call(F, lits=[1, 2, bad, 3])
    assert rc == ERR_ARG and "literal" in msg


def test_empty_batch_is_ok():
    assert _call([])[0] == _capi.OK
    assert _call([], null=("icb", "clb", "lits", "res", "steps", "tr", "sc"))[0] == _capi.OK
    assert eliminate_batch([]) == []
    from satmi import solvers
    assert solvers.davis_putnam_solver_batch([]) == []


def test_debug_knob_arguments():
    try:
        debug_batch(2, 64)
        debug_batch(0, R.CAP_MAX)
        for grid, cap in ((-1, 0), (0, -1), (0, R.CAP_MAX + 1)):
            with pytest.raises(_capi.SatmiError):
                debug_batch(grid, cap)
    finally:
        debug_batch(0, 0)


# ---------------------------------------------------------------- row proofs
def _same_as_oracle(f, **lim):
    """The host restatement of the kernel (slot rule, greedy filter, first event
    in pair order) gives the oracle's elimination of f."""
    o, m = oracle.dp(f, record=True, **lim), R.model(f, **lim)
    n = R.completed(o)
    assert (m["result"], m["vars"], m["steps"]) == (o["result"], o["vars"], o["steps"]), f
    assert m["clauses"] == [[R.lit_order(c) for c in cl] for cl in o["clauses"][:n]], f


def test_rows_edge_cases():
    for f in R.EDGE:
        p = R.profile(f)
        assert R.fits(p) == (f != [[5], [-5, 13]]), f
        if R.fits(p):
            _same_as_oracle(f)
    assert R.profile([[5], [-5, 13]])["collide_step"] == 0


def test_rows_mix():
    fs = R.mix()
    assert len(fs) == 200 and all(max(R.variables(f)) <= 8 for f in fs)
    ps = [R.profile(f) for f in fs]
    assert all(R.fits(p, 512) for p in ps)                       # none is excused
    assert {p["oracle"]["result"] for p in ps} == {0, 1}
    assert sum(len(f) != len({frozenset(c) for c in f}) for f in fs) >= 200 // 7
    assert sum(any(any(-l in c for l in c) for c in f) for f in fs) >= 200 // 11
    for f in fs:
        _same_as_oracle(f)


def test_rows_sparse_mix():
    """The renamed rows of test_dp_batch_gpu.py::test_sparse_ids: ids above 63
    only, and the batched kernel takes every one of them."""
    fs = R.sparse_mix()
    assert len(fs) == 40 and all(min(R.variables(f)) > 63 for f in fs)
    ps = [R.profile(f) for f in fs]
    assert all(R.fits(p, 512) for p in ps)                       # none is excused
    assert max(p["max_list"] for p in ps) == 30
    assert {p["oracle"]["result"] for p in ps} == {0, 1}
    for f in fs:
        _same_as_oracle(f)


def test_rows_capacity():
    """At SMALL_CAP clauses some rows overflow on input, some in a later list, some never."""
    fs = R.capacity_rows()
    ps = [R.profile(f) for f in fs]
    assert all(R.fits(p, 1024) for p in ps)
    cap = R.SMALL_CAP
    kinds = ["input" if len(f) > cap else "later" if p["max_list"] > cap else "fits" for f, p in zip(fs, ps)]
    assert min(kinds.count(k) for k in ("input", "later", "fits")) >= 2
    # a list of exactly the capacity fits
    assert any(p["max_list"] == cap for p in ps) or any(len(f) == cap for f in fs)


def test_rows_slot_order_and_collisions():
    p = R.profile(R.SLOT)
    assert (p["oracle"]["result"], p["oracle"]["vars"]) == (1, [1, 2, 9]) and R.fits(p)   # 9 before 3
    assert [s["rule"] for s in p["steps"]] == p["oracle"]["vars"]
    p = R.profile(R.SLOT37)
    assert R.fits(p) and p["d"] == 6 and [s["rule"] for s in p["steps"]] == p["oracle"]["vars"]
    assert p["oracle"]["vars"] != sorted(p["oracle"]["vars"])
    assert R.profile(R.COLLIDE0)["collide_step"] == 0
    p = R.profile(R.COLLIDE1)
    assert p["collide_step"] == 1 and p["steps"][0]["rule"] == p["oracle"]["vars"][0] and p["d"] <= R.MAXVARS
    for f in (R.SLOT, R.SLOT37):
        _same_as_oracle(f)


@pytest.mark.parametrize("k", [63, 64, 65])
def test_rows_wave_boundaries(k):
    for sign, name in ((1, "pos"), (-1, "neg")):
        p = R.profile(R.WAVE_ROWS[f"{name}{k}"])
        s = p["steps"][0]
        assert R.fits(p, 512) and s["var"] == 1
        assert (s["np"], s["nn"]) == ((k, 1) if sign > 0 else (1, k))
        assert (s["ncl"], s["kept"], s["next"]) == (k + 1, k, k)
        _same_as_oracle(R.WAVE_ROWS[f"{name}{k}"])


@pytest.mark.parametrize("pairs", [R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2500])
def test_rows_chunk_boundaries(pairs):
    f = R.WAVE_ROWS[f"pairs{pairs}"]
    p = R.profile(f)
    s = p["steps"][0]
    assert R.fits(p, 1024) and s["var"] == 1 and s["pairs"] == pairs and s["kept"] > 64
    _same_as_oracle(f)


def test_rows_variable_bound():
    p = R.profile(R.WAVE_ROWS["d31"])
    assert p["d"] == 31 == R.MAXVARS and R.fits(p, 512) and len(p["steps"]) == 30
    assert [s["rule"] for s in p["steps"]] == p["oracle"]["vars"]
    assert {len(s["live"]) for s in p["steps"]} >= {31, 19, 18, 5, 4, 2}     # every table size on the way
    p = R.profile(R.D32)
    assert p["d"] == 32 and not R.fits(p)


def test_rows_limits():
    row = R.limit_rows(R.mix())
    assert row is not None
    f, lo, hi = row
    ev = R.model(f)["events"]
    nr, cnt, empty_at, before = ev[-1]
    assert empty_at is not None and 1 <= before <= cnt and (lo, hi) == (nr + before - 1, nr + before)
    assert oracle.dp(f, clause_limit=lo)["result"] == -1 and oracle.dp(f, clause_limit=hi)["result"] == 0
    assert oracle.dp(f, clause_limit=lo)["steps"] == oracle.dp(f, clause_limit=hi)["steps"] == len(ev)
    for lim in (lo, hi):
        _same_as_oracle(f, clause_limit=lim)
    for sl in (1, 3):
        for g in R.mix()[:40]:
            _same_as_oracle(g, step_limit=sl)


def test_rows_bench_set_sizes():
    """Two formulas of the bench set (the whole set is the GPU test's): the sizes
    the tiers are chosen for, no collision at any step."""
    b = cnf.uniform_ksat(16, 16, 96, 3, seed=7002)
    p = R.profile(b.instance(1))
    assert R.fits(p, 1024) and p["max_list"] == 898 and max(s["pairs"] for s in p["steps"]) == 43450
    assert p["d"] * 96 <= R.CAP_MAX                                          # the tier rule d x m
    assert [s["rule"] for s in p["steps"]] == p["oracle"]["vars"]
