"""CPU: the rows of tests/dpll_paths.py reach the paths of csrc/dpll.hip they
claim, by the oracle's path counters (oracle/sat_oracle.c oracle_dpll_paths),
and together they reach every one.  Conditions on the inputs only: the GPU
side (test_dpll_paths_gpu.py) runs the same rows against the same oracle.
Also here, because they need no GPU: which kernel the dispatch plans for the
shape rows and the long clauses, and what the drop-in solvers make of a status
that decides nothing."""
import ctypes
import operator
import os
import random

import numpy as np
import pytest

import dpll_paths
import oracle
from dpll_paths import (DPLL_PATH_ROWS, EQ, GE, LDS_LIMIT, LONG_ROWS, NARROW_MAX_LEN, PATH_REACHED, PATHS_NEVER,
                        SHAPE_CLASS, SHAPE_ROWS)
from satmi import _capi

OPS = {GE: operator.ge, EQ: operator.eq}
IDS = [r[0] for r in DPLL_PATH_ROWS]


def test_paths_entry_runs_the_same_search():
    """oracle_dpll_paths is oracle_dpll plus counters: same status, solutions, counts and root assignment."""
    for name, _, kwargs, _ in DPLL_PATH_ROWS:
        if name in SHAPE_ROWS and name != "shape_4_waves":
            continue   # three more of the same generator, the oracle's slowest rows
        for mode in ("ref", "sound"):
            k = dict(kwargs, mode=mode)
            plain = oracle.dpll(dpll_paths.row_formula(name), max_solutions=0, **k)
            withp = dict(dpll_paths.row_oracle(name, mode))
            assert set(withp.pop("paths")) == set(oracle.DPLL_PATHS)
            assert withp == plain, (name, mode)


def test_paths_entry_on_random_mixes():
    """... and on the random mixes of test_dpll_gpu.py (same generator), with and
    without a caller's dict; none of them contradicts the oracle's account of the
    kernel's snapshots (`model_mismatch`) or meets a REF-mode decision."""
    rng = random.Random(4)
    conflicts = 0
    for i in range(300):
        n = rng.randint(1, 20)
        f = []
        for _ in range(rng.randint(1, 120)):
            k = rng.randint(1, min(5, n))
            f.append([v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), k)])
        if rng.random() < 0.3:
            f[rng.randrange(len(f))].append(f[0][0] * rng.choice((1, -1)))
        init = [rng.choice((1, -1)) * rng.randint(1, n + 2) for _ in range(rng.randint(0, 4))] if i % 2 else None
        for mode in ("ref", "sound"):
            plain = oracle.dpll(f, mode, node_limit=500, init=init, sol_cap=16)
            withp = oracle.dpll(f, mode, node_limit=500, init=init, sol_cap=16, paths=True)
            paths = withp.pop("paths")
            assert withp == plain, (mode, f, init)
            for counter in PATHS_NEVER:
                assert paths[counter] == 0, (counter, mode, f, init)
            conflicts += plain["counters"]["conflicts"]
    assert conflicts > 300   # the searches did propagate into conflicts


@pytest.mark.parametrize("row", DPLL_PATH_ROWS, ids=IDS)
def test_row_reaches_its_paths(row):
    name, _, _, needs = row
    for mode in (None, "ref", "sound"):
        paths = dpll_paths.row_oracle(name, mode)["paths"]
        if mode is None:
            print(name, {k: v for k, v in paths.items() if v not in (0, -1)})
            assert needs
            for counter, op, value in needs:
                assert OPS[op](paths[counter], value), f"{name}: {counter} = {paths[counter]}, needs {op} {value}"
        for counter in PATHS_NEVER:
            assert paths[counter] == 0, f"{name} {mode}: {counter} = {paths[counter]}"


def test_rows_cover_every_path():
    """Every counter of the oracle is either reached by a row -- required there
    at PATH_REACHED's value or beyond -- or listed as never moved: a counter
    (a path of the kernel) added without a row fails here."""
    assert set(PATH_REACHED) | set(PATHS_NEVER) == set(oracle.DPLL_PATHS)
    assert not set(PATH_REACHED) & set(PATHS_NEVER)
    for counter, reached in PATH_REACHED.items():
        rows = [name for name, _, _, needs in DPLL_PATH_ROWS
                if any(c == counter and v >= reached for c, _, v in needs)]
        assert rows, f"no row is required to reach {counter} >= {reached}"

    # both sides of the boundaries the kernel switches at
    def values(*counters):
        return {v for _, _, _, needs in DPLL_PATH_ROWS for c, op, v in needs if c in counters and op == EQ}
    assert {64, 65, 128, 129} <= values("snapshot_len_max")                    # one, two, three chunks
    assert {63, 64} <= values("emptied_index_max") and {63, 64} <= values("mismatch_index_max")
    assert {63, 64} <= values("empty_clause_first_index_max")
    assert {64, 65} <= values("undo_len_max") and {64, 65} <= values("stamp_drop_len_max")
    assert {4095, 4096} <= values("unit_clause_index_max")                     # the bitmaps' 64 x 64 bits
    assert {4095, 4096} <= values("pure_first_pos_max")
    assert {255, 256, 300} <= values("clause_len_max")                         # Narrow::MAX_LEN
    assert len(set(IDS)) == len(DPLL_PATH_ROWS)
    assert set(LONG_ROWS) == {"long_256", "long_300", "long_300_empty", "long_300_dups"}


def test_stale_library_is_rebuilt_or_refused(tmp_path):
    """oracle.lib() binds oracle_dpll_paths: a library without it is rebuilt once,
    refused if the rebuild does not bring it; so is a caller with another counter list."""
    import subprocess
    L = oracle.lib()
    assert hasattr(L, "oracle_dpll_paths")
    stale = tmp_path / "stale.c"
    stale.write_text("int oracle_dpll(void) { return 0; }\nint oracle_cdcl_paths(void) { return 0; }\n")
    so = str(tmp_path / "liboracle.so")
    subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-fPIC", "-shared", "-o", so, str(stale)], check=True)
    with pytest.raises(RuntimeError, match="oracle_dpll_paths"):
        oracle._open(so, rebuild=lambda: None)
    off = np.zeros(1, dtype=np.int32)
    pc = np.zeros(len(oracle.DPLL_PATHS) + 1, dtype=np.int64)
    i32 = ctypes.POINTER(ctypes.c_int32)
    assert L.oracle_dpll_paths(1, 0, off.ctypes.data_as(i32), off.ctypes.data_as(i32), 0, 0, 0,
                               off.ctypes.data_as(i32), 0, None, 0, None, 0, None, None, None,
                               pc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(pc)) == -3


# ---- the dispatch, asked of the library (no launch, no GPU)
needs_lib = pytest.mark.skipif(not os.path.exists(_capi.LIB_PATH), reason="libsatmi.so not built")


def _plan(policy, shape, mode=_capi.MODE_REF, has_init=False):
    _capi.set_kernel(policy)
    try:
        return _capi.plan(*shape, mode=mode, has_init=has_init)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)


@needs_lib
def test_layout_restatement_is_the_librarys():
    L = _capi.load()
    rng = random.Random(1)
    shapes = [dpll_paths.shape_of(dpll_paths.row_formula(name))[:3] for name in IDS]
    shapes += [(rng.randint(0, 3000), rng.randint(0, 9000), rng.randint(0, 40000)) for _ in range(200)]
    shapes += [(32766, 10, 10), (32767, 10, 10), (10, 65534, 10), (10, 65535, 10), (10, 10, 65535), (10, 10, 65536)]
    for s in shapes:
        want = dpll_paths.lds_bytes(*s)
        assert L.satmi_dpll_lds_bytes(*s) == (want if want <= LDS_LIMIT else 0), s


@needs_lib
@pytest.mark.parametrize("name", list(SHAPE_ROWS))
def test_shape_rows_fall_in_their_class(name):
    """The LDS shape classes of narrow_shape: 4, 2 and 1 waves per workgroup, a
    workgroup's LDS above 64 KiB in the last two (hipFuncSetAttribute), and the
    two shapes either side of the 160 KiB bound."""
    shape = dpll_paths.shape_of(dpll_paths.row_formula(name))
    b = dpll_paths.lds_bytes(*shape[:3])
    wpg = SHAPE_CLASS[name]
    for mode in (_capi.MODE_REF, _capi.MODE_SOUND):
        kern, lds, waves = _plan(_capi.KERNEL_AUTO, shape, mode, has_init=True)   # a caller's dict: no clause kernel
        if wpg == 0:
            assert b > LDS_LIMIT and (kern, lds, waves) == (_capi.KERNEL_WIDE, 256, 32)
            continue
        assert b <= LDS_LIMIT and (kern, lds) == (_capi.KERNEL_GENERAL, b)
        assert dpll_paths.narrow_shape(b) == (wpg, waves)
        assert (b * wpg > 64 * 1024) == (wpg < 4)
    if name == "shape_under_160k":
        over = dpll_paths.shape_of(dpll_paths.row_formula("shape_over_160k"))
        assert LDS_LIMIT - 256 < b and dpll_paths.lds_bytes(*over[:3]) < LDS_LIMIT + 256


@needs_lib
@pytest.mark.parametrize("name", ["long_255"] + list(LONG_ROWS))
def test_long_clauses_plan_the_wide_form(name):
    """A clause past the LDS form's 255 literals: AUTO plans the wide form although
    the sizes fit the LDS layout; KERNEL_GENERAL stays pinned to the LDS form
    (whose kernel then answers TOO_LARGE for the instance); a length of 0 is
    `unknown` and plans by the sizes alone."""
    shape = dpll_paths.shape_of(dpll_paths.row_formula(name))
    assert 0 < dpll_paths.lds_bytes(*shape[:3]) <= LDS_LIMIT
    long = shape[3] > NARROW_MAX_LEN
    assert long == (name != "long_255")
    for mode in (_capi.MODE_REF, _capi.MODE_SOUND):
        for has_init in (False, True):
            want = _capi.KERNEL_WIDE if long else _capi.KERNEL_GENERAL
            assert _plan(_capi.KERNEL_AUTO, shape, mode, has_init)[0] == want, (mode, has_init)
            assert _plan(_capi.KERNEL_GENERAL, shape, mode, has_init)[0] == _capi.KERNEL_GENERAL
            assert _plan(_capi.KERNEL_WIDE, shape, mode, has_init)[0] == _capi.KERNEL_WIDE
            assert _plan(_capi.KERNEL_AUTO, shape[:3] + (0,), mode, has_init)[0] == _capi.KERNEL_GENERAL


# ---- the drop-in solvers never read a verdict out of a status that decides nothing
def _fake_result(status, nsol=0):
    from satmi.dpll import DpllResult
    counters = np.zeros((1, _capi.NCOUNTERS), dtype=np.int64)
    counters[0, 5] = nsol
    return DpllResult(np.array([status], dtype=np.int32), counters, np.ones((1, 1), dtype=np.int32),
                      np.ones((1, 1, 1), dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros((1, 1), dtype=np.int32))


@pytest.mark.parametrize("status", [_capi.DPLL_TOO_LARGE, _capi.DPLL_NODE_LIMIT, 9])
def test_dpll_solve_raises_on_an_undecided_status(monkeypatch, status):
    from satmi import solvers
    monkeypatch.setattr(solvers, "dpll_batch", lambda *a, **k: _fake_result(status))
    with pytest.raises(_capi.SatmiError, match="status"):
        solvers.dpll_solve([[1, 2]])
    with pytest.raises(_capi.SatmiError, match="status"):
        solvers.dpll_optimized([[1, 2]])


def test_dpll_solve_verdicts_and_timeout(monkeypatch):
    from satmi import solvers
    monkeypatch.setattr(solvers, "dpll_batch", lambda *a, **k: _fake_result(_capi.DPLL_TIMEOUT))
    with pytest.raises(solvers.SolverTimeout):
        solvers.dpll_solve([[1, 2]])
    monkeypatch.setattr(solvers, "dpll_batch", lambda *a, **k: _fake_result(_capi.DPLL_EXHAUSTED))
    assert solvers.dpll_solve([[1], [-1]]) == (False, None)
    monkeypatch.setattr(solvers, "dpll_batch", lambda *a, **k: _fake_result(_capi.DPLL_STOPPED, nsol=1))
    assert solvers.dpll_solve([[1]]) == (True, {1: True})
