"""CPU checks of satmi_cdcl_sound_batch_host's refusals through the C ABI, in the manner of
tests/test_dpll_refute_args.py: the batch goes through batch_keys.h before any HIP call, so
every refusal below comes back without a GPU, under the entry point's name, with the cause
named and the outputs untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

from satmi import _capi
from satmi.refute import proof_of_cdcl

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_cdcl_sound_batch_host"
I32_MIN = -(2 ** 31)

# three formulas, the middle one empty
ICB, CLB, LITS, NV = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6], [3, 0, 6]
B, STRIDE, CCAP, LCAP = 3, 6, 8, 16
INPUTS = ("icb", "clb", "lits", "nv")
OUTPUTS = ("status", "counters", "row_len", "row_lits", "pib", "pcb", "plits", "info", "totals")
I64 = ("counters", "info", "totals")


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_int32))


def _call(count=B, ccap=CCAP, lcap=LCAP, room_cap=0, stride=STRIDE, null=(), **over):
    """The host form on the arrays above, those in `over` replaced and those named in `null`
    passed as NULL -> (return code, message, outputs), the outputs pre-filled with SENTINEL."""
    a = dict(zip(INPUTS, (ICB, CLB, LITS, NV)))
    a.update(over)
    a = {k: None if k in null else np.array(v, dtype=np.int64).astype(np.int32) for k, v in a.items()}
    sizes = dict(status=B, counters=B * 8, row_len=B, row_lits=B * 8192, pib=B + 1, pcb=CCAP + 1, plits=LCAP,
                 info=B * _capi.CDCL_SOUND_NWORDS, totals=2)
    o = {k: np.full(n, SENTINEL, np.int64 if k in I64 else np.int32) for k, n in sizes.items()}
    q = {k: None if k in null else v for k, v in o.items()}
    L = _capi.load()
    rc = L.satmi_cdcl_sound_batch_host(
        count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["nv"]), 0, 0.0, room_cap, _p(q["status"]),
        _p(q["counters"]), _p(q["row_len"]), _p(q["row_lits"]), stride, _p(q["pib"]), _p(q["pcb"]), ccap,
        _p(q["plits"]), lcap, _p(q["info"]), _p(q["totals"]))
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o


def _refused(rc, msg, o, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert all((v == SENTINEL).all() for v in o.values())


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "satmi.h")).read()
    defs = dict(re.findall(r"#define (SATMI_CDCL_SOUND_[A-Z_]+) (\d+)", text))
    for name in ("UNSAT", "SAT", "LIMIT", "FULL", "TOO_LARGE", "NCOUNTERS", "NWORDS", "TRUNCATED", "MAX_VARS"):
        assert int(defs["SATMI_CDCL_SOUND_" + name]) == getattr(_capi, "CDCL_SOUND_" + name), name
    assert len(_capi.CDCL_SOUND_COUNTERS) == _capi.CDCL_SOUND_NCOUNTERS
    assert len(_capi.CDCL_SOUND_WORDS) == _capi.CDCL_SOUND_NWORDS
    assert _capi.CDCL_SOUND_MAX_VARS <= _capi.TRIM_MAX_VARS      # every proof can be checked and trimmed
    assert _capi.load().satmi_abi_version() == 2


def test_lds_bytes_query():
    L = _capi.load()
    at_limit = L.satmi_cdcl_sound_lds_bytes(_capi.CDCL_SOUND_MAX_VARS)
    assert 0 < at_limit <= 160 * 1024 and at_limit % 16 == 0
    assert 0 < L.satmi_cdcl_sound_lds_bytes(50) < 1024
    assert L.satmi_cdcl_sound_lds_bytes(_capi.CDCL_SOUND_MAX_VARS + 1) == 0 and L.satmi_cdcl_sound_lds_bytes(-1) == 0


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


@pytest.mark.parametrize("name", ("status", "counters", "row_len", "row_lits", "pib", "pcb", "plits", "totals"))
def test_null_output_pointers(name):
    """(h_info alone may be NULL, by the header: an output the caller does not want.)"""
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


@pytest.mark.parametrize("ccap,lcap", [(2 ** 31 - 1, LCAP), (CCAP, 2 ** 31), (2 ** 40, 2 ** 40)])
def test_capacities_beyond_the_32_bit_offsets(ccap, lcap):
    """proof_clause_begin holds capacity + 1 int32 offsets into proof_lits: at most 2^31 - 2
    lemmas and 2^31 - 1 literals (refused before the arrays, far smaller here, are touched)."""
    _refused(*_call(ccap=ccap, lcap=lcap), "proof capacity beyond the 32-bit offsets")


def test_room_cap_and_row_stride():
    _refused(*_call(room_cap=-1), "negative room_cap")
    _refused(*_call(stride=0), "row stride < 1")
    _refused(*_call(stride=5), "row stride < number of variables")


def test_past_the_variable_limit_is_too_large_before_any_launch():
    """One variable beyond SATMI_CDCL_SOUND_MAX_VARS: SATMI_ERR_TOO_LARGE without a GPU, by a
    literal or by inst_nvars alone; the limit itself passes the check (and then needs a GPU,
    which this test does not ask for)."""
    top = _capi.CDCL_SOUND_MAX_VARS + 1
    lits = list(LITS)
    lits[8] = -top
    _refused(*_call(lits=lits, nv=[3, 0, top], stride=top), f"variable {top} is beyond the layout's {top - 1}",
             code=ERR_TOO_LARGE)
    _refused(*_call(nv=[3, top, 6], stride=top), "beyond the layout's", code=ERR_TOO_LARGE)


def test_device_forms_refuse_what_they_can_see():
    """satmi_cdcl_sound_batch_device and satmi_cdcl_sound_pack_device refuse before they touch the device."""
    L = _capi.load()
    p = 4096   # never dereferenced

    def solve(n=1, max_vars=3, mlen=3, stride=3, ptrs=None):
        q = ptrs or [p] * 11
        return L.satmi_cdcl_sound_batch_device(n, q[0], q[1], q[2], q[3], max_vars, mlen, 0, 0.0, q[4], q[5], q[6],
                                               q[7], q[8], q[9], stride, q[10], None)

    def packed(n=1, ccap=4, lcap=4, ptrs=None):
        q = ptrs or [p] * 8
        return L.satmi_cdcl_sound_pack_device(n, q[0], q[1], q[2], q[3], q[4], q[5], ccap, q[6], lcap, q[7], None)
    assert solve(n=-1) == ERR_ARG and "negative formula count" in L.satmi_last_error().decode()
    assert solve(max_vars=-1) == ERR_ARG and solve(mlen=-1) == ERR_ARG and solve(stride=0) == ERR_ARG
    assert solve(n=0) == _capi.OK and packed(n=0) == _capi.OK
    assert solve(max_vars=_capi.CDCL_SOUND_MAX_VARS + 1) == ERR_TOO_LARGE
    assert "satmi_cdcl_sound_batch_device: variable 8192" in L.satmi_last_error().decode()
    for null in range(11):
        q = [p] * 11
        q[null] = None
        assert solve(ptrs=q) == ERR_ARG, null
        assert "null pointer" in L.satmi_last_error().decode()
    assert packed(n=-1) == ERR_ARG and packed(ccap=0) == ERR_ARG and packed(lcap=0) == ERR_ARG
    assert "non-positive proof capacity" in L.satmi_last_error().decode()
    for null in range(8):
        q = [p] * 8
        q[null] = None
        assert packed(ptrs=q) == ERR_ARG, null
        assert "satmi_cdcl_sound_pack_device: null pointer" in L.satmi_last_error().decode()


def test_debug_knob_arguments():
    L = _capi.load()
    assert L.satmi_cdcl_sound_debug_grid(-1, 1) == ERR_ARG and L.satmi_cdcl_sound_debug_grid(1, 3) == ERR_ARG
    assert L.satmi_cdcl_sound_debug_room(-1) == ERR_ARG
    assert L.satmi_cdcl_sound_debug_grid(0, 0) == _capi.OK and L.satmi_cdcl_sound_debug_room(0) == _capi.OK


def test_proof_of_cdcl_arguments():
    with pytest.raises(ValueError, match="no refutation"):
        proof_of_cdcl({"sat": True, "proof": None})
    with pytest.raises(ValueError, match="no refutation"):
        proof_of_cdcl({"sat": None, "proof": None})
    assert proof_of_cdcl({"sat": False, "proof": [(1,), ()]}) == [[1], []]
