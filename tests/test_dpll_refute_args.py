"""CPU checks of satmi_dpll_refutations_host's refusals through the C ABI, in the manner
of tests/test_refute_args.py: the batch goes through batch_keys.h before any HIP call, so
every refusal below comes back without a GPU, under the entry point's name, with the
cause named and the outputs untouched."""
import ctypes

import numpy as np
import pytest

from satmi import _capi
from satmi.refute import dpll_refutations, dpll_refutations_packed, proof_of_dpll
from satmi.cnf import pack

ERR_ARG = -1
SENTINEL = 77
WHO = "satmi_dpll_refutations_host"
I32_MIN = -(2 ** 31)

# three formulas, the middle one empty
ICB, CLB, LITS, NV = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6], [3, 0, 6]
B, STRIDE, CCAP, LCAP = 3, 6, 8, 16
INPUTS = ("icb", "clb", "lits", "nv")
OUTPUTS = ("status", "counters", "sol_len", "sol_lits", "root_len", "root_lits", "pib", "pcb", "plits", "info", "totals")
I64 = ("counters", "info", "totals")


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_int32))


def _call(count=B, ccap=CCAP, lcap=LCAP, sol_cap=1, stride=STRIDE, null=(), **over):
    """The host form on the arrays above, those in `over` replaced and those named in `null`
    passed as NULL -> (return code, message, outputs), the outputs pre-filled with SENTINEL."""
    a = dict(zip(INPUTS, (ICB, CLB, LITS, NV)))
    a.update(over)
    a = {k: None if k in null else np.array(v, dtype=np.int64).astype(np.int32) for k, v in a.items()}
    sizes = dict(status=B, counters=B * 8, sol_len=B, sol_lits=B * STRIDE, root_len=B, root_lits=B * STRIDE,
                 pib=B + 1, pcb=CCAP + 1, plits=LCAP, info=B * _capi.DPLL_PROOF_NWORDS, totals=2)
    o = {k: np.full(n, SENTINEL, np.int64 if k in I64 else np.int32) for k, n in sizes.items()}
    q = {k: None if k in null else v for k, v in o.items()}
    L = _capi.load()
    rc = L.satmi_dpll_refutations_host(
        count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["nv"]), 1, 0, 0.0, sol_cap, stride,
        _p(q["status"]), _p(q["counters"]), _p(q["sol_len"]), _p(q["sol_lits"]), _p(q["root_len"]),
        _p(q["root_lits"]), _p(q["pib"]), _p(q["pcb"]), ccap, _p(q["plits"]), lcap, _p(q["info"]), _p(q["totals"]))
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o


def _refused(rc, msg, o, *words):
    assert rc == ERR_ARG, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert all((v == SENTINEL).all() for v in o.values())


def test_constants_match_the_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "satmi.h")).read()
    defs = dict(re.findall(r"#define (SATMI_DPLL_PROOF_[A-Z]+) (\d+)", text))
    assert int(defs["SATMI_DPLL_PROOF_NWORDS"]) == _capi.DPLL_PROOF_NWORDS == len(_capi.DPLL_PROOF_WORDS)
    assert int(defs["SATMI_DPLL_PROOF_TRUNCATED"]) == _capi.DPLL_PROOF_TRUNCATED
    assert _capi.load().satmi_abi_version() == 2


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_empty_batch_is_ok():
    """B = 0 returns SATMI_OK whatever the pointers are, and touches nothing."""
    for null in ((), INPUTS + OUTPUTS):
        rc, _, o = _call(count=0, null=null)
        assert rc == _capi.OK and all((v == SENTINEL).all() for v in o.values())


@pytest.mark.parametrize("name", INPUTS)
def test_null_input_pointers(name):
    _refused(*_call(null=(name,)), "null pointer")


@pytest.mark.parametrize("name", ("status", "counters", "pib", "pcb", "plits", "totals"))
def test_null_output_pointers(name):
    _refused(*_call(null=(name,)), "null pointer")


@pytest.mark.parametrize("over,words", [
    (dict(icb=[0, 2, 1, 5]), ("clause ranges are not ascending",)),
    (dict(icb=[-1, 2, 2, 5]), ("clause ranges are not ascending",)),
    (dict(clb=[0, 2, 1, 6, 7, 9]), ("literal ranges are not ascending",)),
    (dict(clb=[-1, 2, 3, 6, 7, 9]), ("literal ranges are not ascending",)),
    (dict(nv=[3, -1, 6]), ("negative inst_nvars",)),
    (dict(nv=[3, 0, 5]), ("literal beyond inst_nvars",)),
])
def test_ranges_that_do_not_ascend_and_variable_counts(over, words):
    _refused(*_call(**over), *words)


@pytest.mark.parametrize("bad", [0, I32_MIN])
@pytest.mark.parametrize("at", [0, 8])
def test_literals_without_a_variable(at, bad):
    lits = list(LITS)
    lits[at] = bad
    _refused(*_call(lits=lits), "literal 0 / INT32_MIN")


@pytest.mark.parametrize("ccap,lcap", [(0, LCAP), (CCAP, 0), (-1, LCAP), (CCAP, -5), (0, 0)])
def test_non_positive_capacities(ccap, lcap):
    _refused(*_call(ccap=ccap, lcap=lcap), "non-positive proof capacity")


def test_solution_buffer_arguments():
    _refused(*_call(sol_cap=-1), "negative sol_cap")
    _refused(*_call(stride=5), "sol_stride < number of variables")


def test_device_form_refuses_what_it_can_see():
    """satmi_dpll_refutations_device refuses before it touches the device."""
    L = _capi.load()
    p = 4096   # never dereferenced

    def call(n=1, ccap=4, lcap=4, sol_cap=1, stride=3, ptrs=None):
        q = ptrs or [p] * 18
        return L.satmi_dpll_refutations_device(n, q[0], q[1], q[2], q[3], 3, 3, 9, 3, 1, 0, 0.0, sol_cap, stride,
                                               q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], ccap,
                                               q[14], lcap, q[15], q[16], None)
    assert call(n=-1) == ERR_ARG and "negative formula count" in L.satmi_last_error().decode()
    assert call(ccap=0) == ERR_ARG and call(lcap=0) == ERR_ARG
    assert "non-positive proof capacity" in L.satmi_last_error().decode()
    assert call(sol_cap=-1) == ERR_ARG and call(stride=2) == ERR_ARG
    assert call(n=0) == _capi.OK
    for null in (0, 1, 3, 4, 5, 10, 11, 12, 13, 14, 15, 16):
        q = [p] * 18
        q[null] = None
        assert call(ptrs=q) == ERR_ARG, null
        assert "null pointer" in L.satmi_last_error().decode()


def test_python_wrapper_arguments():
    """Logging needs SOUND mode and no caller assignment: refused as SATMI_ERR_ARG, before
    anything is launched."""
    f = [[[1, 2], [-1]]]
    for kw in (dict(mode="ref"), dict(inits=[[1]]), dict(mode="ref", inits=[[]])):
        with pytest.raises(_capi.SatmiError, match=r"\(-1\).*SOUND mode and no caller assignment"):
            dpll_refutations(f, **kw)
        with pytest.raises(_capi.SatmiError, match=r"\(-1\)"):
            dpll_refutations_packed(pack(f), **kw)
    with pytest.raises(ValueError, match="literal 0"):
        dpll_refutations([[[0]]])
    with pytest.raises(ValueError, match="no refutation"):
        proof_of_dpll({"sat": True, "proof": None})
    assert proof_of_dpll({"sat": False, "proof": [(1,), ()]}) == [[1], []]
