"""CPU checks of the batched resolution entry point (csrc/resolution_batch.hip):
satmi_resolution_batch_host validates its arguments before any HIP call, so
every return below comes back without a GPU."""
import ctypes

import numpy as np
import pytest

from satmi import _capi
from satmi.resolution import debug_batch, resolve_batch

ERR_ARG = -1
I32_MIN = -(2 ** 31)


def _p(a, t=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _call(formulas, num=None, pass_cap=4, null=(), lits=None):
    """satmi_resolution_batch_host on `formulas` (literals overridden by `lits`), the
    arguments named in `null` passed as NULL -> (return code, message)."""
    L = _capi.load()
    icb = np.cumsum([0] + [len(f) for f in formulas]).astype(np.int32)
    clb = np.cumsum([0] + [len(c) for f in formulas for c in f]).astype(np.int32)
    flat = [l for f in formulas for c in f for l in c] if lits is None else lits
    la = np.array(flat or [0], dtype=np.int64).astype(np.int32)
    B = len(formulas) if num is None else num
    res = np.full(max(B, 1), 7, dtype=np.int32)
    passes = np.full(max(B, 1), 7, dtype=np.int32)
    pn = np.zeros(max(B, 1) * max(pass_cap, 1), dtype=np.int64)
    a = {"icb": _p(icb), "clb": _p(clb), "lits": _p(la), "res": _p(res), "passes": _p(passes),
         "pn": _p(pn, ctypes.c_int64)}
    for k in null:
        a[k] = None
    rc = L.satmi_resolution_batch_host(B, a["icb"], a["clb"], a["lits"], 0, 0, a["res"], a["passes"], a["pn"],
                                       pass_cap, None, 0, None, 0, None)
    return rc, (L.satmi_last_error() or b"").decode()


F = [[[1, 2], [-1]], [[3]]]


def test_negative_count():
    rc, msg = _call(F, num=-1)
    assert rc == ERR_ARG and "satmi_resolution_batch_host" in msg


def test_negative_pass_cap():
    rc, msg = _call(F, pass_cap=-1)
    assert rc == ERR_ARG and "pass_cap" in msg


@pytest.mark.parametrize("name", ["icb", "clb", "lits", "res", "passes", "pn"])
def test_null_required_pointer(name):
    rc, msg = _call(F, null=(name,))
    assert rc == ERR_ARG and "null" in msg


@pytest.mark.parametrize("bad", [0, I32_MIN])
def test_bad_literal(bad):
    rc, msg = _call(F, lits=[1, 2, bad, 3])
    assert rc == ERR_ARG and "literal" in msg


def test_empty_batch_is_ok():
    assert _call([])[0] == _capi.OK
    assert _call([], null=("icb", "clb", "lits", "res", "passes", "pn"))[0] == _capi.OK


def test_resolve_batch_of_nothing():
    assert resolve_batch([]) == []


def test_debug_knob_arguments():
    try:
        debug_batch(2, 64)
        debug_batch(0, 4096)
        for grid, cap in ((-1, 0), (0, -1), (0, 4097)):
            with pytest.raises(_capi.SatmiError):
                debug_batch(grid, cap)
    finally:
        debug_batch(0, 0)


def test_solvers_export():
    from satmi import solvers
    assert solvers.resolution_solver_batch([]) == []
