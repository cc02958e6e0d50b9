"""CPU checks of the four older entry points that take CSR host arrays
(satmi_dpll_batch_host, satmi_cdcl_batch_host, satmi_dp_host,
satmi_resolution_host): each validates its arrays through batch_keys.h before
any HIP call, so every refusal below comes back without a GPU, under the entry
point's name, with the cause named and the outputs untouched.  (The two
single-formula entry points reset *result and *steps / *passes before they
look at the literals, as they always did: a refused literal leaves -1 and 0.)"""
import ctypes

import numpy as np
import pytest

from satmi import _capi

ERR_ARG = -1
I32_MIN = -(2 ** 31)
SENTINEL = 77

# three formulas of at most six variables, the middle one empty; the
# single-formula entry points take their five clauses as one formula
F = [[[1, -2], [3]], [], [[-4, 5, 6], [2], [-1, -6]]]
ICB = [0, 2, 2, 5]
CLB = [0, 2, 3, 6, 7, 9]
LITS = [1, -2, 3, -4, 5, 6, 2, -1, -6]
NVARS = [3, 0, 6]
BATCHED = ("satmi_dpll_batch_host", "satmi_cdcl_batch_host")
SINGLE = ("satmi_dp_host", "satmi_resolution_host")
ENTRIES = BATCHED + SINGLE
REQUIRED = {
    "satmi_dpll_batch_host": ("icb", "clb", "lits", "nvars"),
    "satmi_cdcl_batch_host": ("icb", "clb", "lits", "status", "alen", "assign", "stats", "vinc"),
    "satmi_dp_host": ("clb", "lits", "result", "count"),
    "satmi_resolution_host": ("clb", "lits", "result", "count"),
}


def _p(a, t=ctypes.c_int32):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def _i32(x):
    return np.array(x, dtype=np.int64).astype(np.int32)


def _call(entry, count=None, null=(), all_null=False, **over):
    """`entry` on F with the arrays in `over` replaced (icb, clb, lits, nvars, init_begin,
    init_lits) and the arguments named in `null` passed as NULL -> (return code, message,
    the output arrays by name, each pre-filled with SENTINEL)."""
    L = _capi.load()
    B, C = len(F), len(CLB) - 1
    a = {"icb": _i32(over.get("icb", ICB)), "clb": _i32(over.get("clb", CLB)), "lits": _i32(over.get("lits", LITS)),
         "nvars": _i32(over.get("nvars", NVARS)),
         "init_begin": _i32(over["init_begin"]) if "init_begin" in over else None,
         "init_lits": _i32(over["init_lits"]) if "init_lits" in over else None}
    if entry == "satmi_dpll_batch_host":
        outs = {"status": np.full(B, SENTINEL, np.int32), "counters": np.full(B * _capi.NCOUNTERS, SENTINEL, np.int64),
                "sol_len": np.full(B, SENTINEL, np.int32), "sol_lits": np.full(B * 6, SENTINEL, np.int32),
                "root_len": np.full(B, SENTINEL, np.int32), "root_lits": np.full(B * 6, SENTINEL, np.int32)}
    elif entry == "satmi_cdcl_batch_host":
        outs = {"status": np.full(B, SENTINEL, np.int32), "alen": np.full(B, SENTINEL, np.int32),
                "assign": np.full(B * 6, SENTINEL, np.int32), "stats": np.full(B * 8, SENTINEL, np.int64),
                "vinc": np.full(B, float(SENTINEL), np.float64)}
    else:
        outs = {"result": np.full(1, SENTINEL, np.int32), "count": np.full(1, SENTINEL, np.int32),
                "trace": np.full(8, SENTINEL, np.int32), "pass_new": np.full(8, SENTINEL, np.int64)}
    a.update(outs)
    for k in (a if all_null else null):
        a[k] = None
    p = {k: _p(v, {np.dtype(np.int64): ctypes.c_int64, np.dtype(np.float64): ctypes.c_double}.get(
        getattr(v, "dtype", None), ctypes.c_int32)) for k, v in a.items()}
    if entry == "satmi_dpll_batch_host":
        rc = L.satmi_dpll_batch_host(B if count is None else count, p["icb"], p["clb"], p["lits"], p["nvars"],
                                     p["init_begin"], p["init_lits"], over.get("mode", _capi.MODE_SOUND), 1, 0, 0.0,
                                     1, 6, p["status"], p["counters"], p["sol_len"], p["sol_lits"], p["root_len"],
                                     p["root_lits"])
    elif entry == "satmi_cdcl_batch_host":
        rc = L.satmi_cdcl_batch_host(B if count is None else count, p["icb"], p["clb"], p["lits"], 0, 0, 0.0,
                                     p["status"], p["alen"], p["assign"], over.get("assign_stride", 6), p["stats"],
                                     p["vinc"])
    elif entry == "satmi_dp_host":
        rc = L.satmi_dp_host(C if count is None else count, p["clb"], p["lits"], 0, 0, 0.0, p["result"], p["trace"], 8,
                             p["count"], None, 0, None, 0, None, 0)
    else:
        rc = L.satmi_resolution_host(C if count is None else count, p["clb"], p["lits"], 0, 0, 0.0, p["result"],
                                     p["count"], p["pass_new"], 8, None, 0, None, 0, None, 0)
    return rc, (L.satmi_last_error() or b"").decode(), outs


def _refused(entry, cause, reset=False, **kw):
    """The call is SATMI_ERR_ARG under the entry point's name with `cause` named, and wrote no
    output (`reset`: but for what a single-formula entry point resets before it reads literals)."""
    rc, msg, outs = _call(entry, **kw)
    assert rc == ERR_ARG and msg.startswith(entry + ": ") and cause in msg, (rc, msg)
    for name, arr in outs.items():
        if reset and name in ("result", "count"):
            assert arr.tolist() == [-1 if name == "result" else 0], (name, arr)
        else:
            assert (arr == SENTINEL).all(), (name, arr)


def _descending(arr, at):
    out = list(arr)
    out[at] = -1 if at == 0 else out[at - 1] - 1
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_negative_count(entry):
    _refused(entry, "negative formula count" if entry in BATCHED else "negative clause count", count=-1)


@pytest.mark.parametrize("entry,name", [(e, n) for e in ENTRIES for n in REQUIRED[e]])
def test_null_required_pointer(entry, name):
    _refused(entry, "null pointer", null=(name,))


@pytest.mark.parametrize("at", [0, 1, 2, 3])   # below 0; descending first, in the middle, last
@pytest.mark.parametrize("entry", BATCHED)
def test_clause_ranges_not_ascending(entry, at):
    _refused(entry, "clause ranges are not ascending", icb=_descending(ICB, at))


@pytest.mark.parametrize("at", [0, 1, 3, 5])
@pytest.mark.parametrize("entry", ENTRIES)
def test_literal_ranges_not_ascending(entry, at):
    _refused(entry, "literal ranges are not ascending", clb=_descending(CLB, at))


@pytest.mark.parametrize("at", [0, 4, 8])
@pytest.mark.parametrize("bad", [0, I32_MIN])
@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_literal(entry, bad, at):
    lits = list(LITS)
    lits[at] = bad
    _refused(entry, "literal 0 / INT32_MIN", reset=entry in SINGLE, lits=lits)


@pytest.mark.parametrize("entry", BATCHED)
def test_empty_batch_is_ok(entry):
    for all_null in (False, True):
        rc, _, outs = _call(entry, count=0, all_null=all_null)
        assert rc == _capi.OK
        assert all((arr == SENTINEL).all() for arr in outs.values())


def test_empty_formula_is_ok():
    """No clause: Davis-Putnam's `while variables` never runs -- True, with neither array read.
    (Resolution takes its workspace even then: tests/test_host_layout_gpu.py.)"""
    rc, _, outs = _call("satmi_dp_host", count=0, null=("clb", "lits"))
    assert rc == _capi.OK and outs["result"].tolist() == [1] and outs["count"].tolist() == [0]


def test_cdcl_negative_assign_stride():
    _refused("satmi_cdcl_batch_host", "negative assign_stride", assign_stride=-1)
    _refused("satmi_cdcl_batch_host", "assign_stride < number of variables", assign_stride=5)


# ---- satmi_dpll_batch_host's own rules
DPLL = "satmi_dpll_batch_host"


@pytest.mark.parametrize("b", [0, 1, 2])
def test_dpll_negative_inst_nvars(b):
    nv = list(NVARS)
    nv[b] = -1
    _refused(DPLL, "negative inst_nvars", nvars=nv)


@pytest.mark.parametrize("b,nv", [(0, 2), (2, 5)])
def test_dpll_literal_beyond_inst_nvars(b, nv):
    """A literal one past inst_nvars[b] would index past the LDS image the kernel sizes from it."""
    nvars = list(NVARS)
    nvars[b] = nv
    _refused(DPLL, "literal beyond inst_nvars", nvars=nvars)


@pytest.mark.parametrize("at", [0, 1, 2, 3])
def test_dpll_init_ranges_not_ascending(at):
    _refused(DPLL, "init ranges are not ascending", init_begin=_descending([0, 1, 1, 3], at), init_lits=[1, -4, 5])


@pytest.mark.parametrize("bad", [0, I32_MIN])
@pytest.mark.parametrize("at", [0, 2])
def test_dpll_bad_init_literal(bad, at):
    lits = [1, -4, 5]
    lits[at] = bad
    _refused(DPLL, "init literal 0 / INT32_MIN", init_begin=[0, 1, 1, 3], init_lits=lits)


def test_dpll_null_init_literals():
    _refused(DPLL, "null pointer", init_begin=[0, 1, 1, 3])
    _refused(DPLL, "sol_stride < number of variables", init_begin=[0, 1, 1, 3], init_lits=[1, -4, 7])


@pytest.mark.parametrize("mode", ["MODE_REF", "MODE_SOUND"])
def test_dpll_refuses_in_both_modes(mode):
    _refused(DPLL, "literal 0 / INT32_MIN", lits=[0] + LITS[1:], mode=getattr(_capi, mode))
