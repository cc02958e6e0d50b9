"""CPU checks of satmi_cdcl_assume_batch_host's refusals through the C ABI, in the manner of
tests/test_cdcl_sound_args.py: the batch goes through batch_keys.h and the assumption arrays
through their own check before any HIP call, so every refusal below comes back without a GPU,
under the entry point's name, with the cause named and the outputs untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

from satmi import _capi, cdcl_sound
from satmi.refute import proof_of_cdcl_assumed

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_cdcl_assume_batch_host"
I32_MIN = -(2 ** 31)

# three formulas, the middle one empty; the first assumes two literals, the last one
ICB, CLB, LITS, NV = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6], [3, 0, 6]
AB, AL = [0, 2, 2, 3], [3, -1, 6]
B, STRIDE, CCAP, LCAP, CSTRIDE = 3, 6, 8, 16, 2
INPUTS = ("icb", "clb", "lits", "nv", "ab", "al")
OUTPUTS = ("status", "counters", "row_len", "row_lits", "pib", "pcb", "plits", "info", "totals", "core_len", "core_lits")
I64 = ("counters", "info", "totals")


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_int32))


def _call(count=B, ccap=CCAP, lcap=LCAP, room_cap=0, stride=STRIDE, core_stride=CSTRIDE, null=(), **over):
    """The host form on the arrays above, those in `over` replaced and those named in `null`
    passed as NULL -> (return code, message, outputs), the outputs pre-filled with SENTINEL."""
    a = dict(zip(INPUTS, (ICB, CLB, LITS, NV, AB, AL)))
    a.update(over)
    a = {k: None if k in null else np.array(v, dtype=np.int64).astype(np.int32) for k, v in a.items()}
    sizes = dict(status=B, counters=B * 8, row_len=B, row_lits=B * 8192, pib=B + 1, pcb=CCAP + 1, plits=LCAP,
                 info=B * _capi.CDCL_SOUND_NWORDS, totals=2, core_len=B, core_lits=B * 8)
    o = {k: np.full(n, SENTINEL, np.int64 if k in I64 else np.int32) for k, n in sizes.items()}
    q = {k: None if k in null else v for k, v in o.items()}
    L = _capi.load()
    rc = L.satmi_cdcl_assume_batch_host(
        count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["nv"]), 0, 0.0, room_cap, _p(q["status"]),
        _p(q["counters"]), _p(q["row_len"]), _p(q["row_lits"]), stride, _p(q["pib"]), _p(q["pcb"]), ccap,
        _p(q["plits"]), lcap, _p(q["info"]), _p(q["totals"]), _p(a["ab"]), _p(a["al"]), _p(q["core_len"]),
        _p(q["core_lits"]), core_stride)
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o


def _refused(rc, msg, o, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert all((v == SENTINEL).all() for v in o.values())


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "satmi.h")).read()
    defs = dict(re.findall(r"#define (SATMI_CDCL_SOUND_[A-Z_]+) (\d+)", text))
    assert int(defs["SATMI_CDCL_SOUND_ASSUMED"]) == _capi.CDCL_SOUND_ASSUMED == 5
    assert _capi.CDCL_SOUND_STATUS_NAMES[_capi.CDCL_SOUND_ASSUMED] == "assumed"
    assert _capi.load().satmi_abi_version() == 2


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_empty_batch_is_ok():
    for null in ((), INPUTS + OUTPUTS):
        rc, _, o = _call(count=0, null=null)
        assert rc == _capi.OK and all((v == SENTINEL).all() for v in o.values())


@pytest.mark.parametrize("name", INPUTS)
def test_null_input_pointers(name):
    """(assume_begin among them: the assumption-carrying form has no "no assumptions" pointer.)"""
    _refused(*_call(null=(name,)), "null pointer")


@pytest.mark.parametrize("name", [n for n in OUTPUTS if n != "info"])
def test_null_output_pointers(name):
    _refused(*_call(null=(name,)), "null pointer")


def test_core_lits_may_be_null_only_without_a_stride():
    """With core_stride = 0 no core literal is written: the check lets a NULL h_core_lits
    through, and the next refusal is another one's."""
    _refused(*_call(null=("core_lits",), core_stride=0, room_cap=-1), "negative room_cap")
    _refused(*_call(null=("core_lits",), core_stride=0, nv=[3, -1, 6]), "negative inst_nvars")
    _refused(*_call(null=("core_lits",), core_stride=1), "null pointer")


@pytest.mark.parametrize("over,words", [
    (dict(icb=[0, 2, 1, 5]), ("clause ranges are not ascending",)),
    (dict(clb=[0, 2, 1, 6, 7, 9]), ("literal ranges are not ascending",)),
    (dict(nv=[3, -1, 6]), ("negative inst_nvars",)),
    (dict(nv=[3, 0, 5]), ("literal beyond inst_nvars",)),
    (dict(ab=[0, 2, 1, 3]), ("assumption ranges are not ascending",)),
    (dict(ab=[-1, 2, 2, 3]), ("assumption ranges are not ascending",)),
    (dict(ab=[0, 3, 3, 2]), ("assumption ranges are not ascending",)),
    (dict(al=[3, 0, 6]), ("assumption literal 0 / INT32_MIN",)),
    (dict(al=[3, -1, I32_MIN]), ("assumption literal 0 / INT32_MIN",)),
    (dict(al=[4, -1, 6]), ("assumption literal beyond inst_nvars",)),
    (dict(al=[3, -1, -7]), ("assumption literal beyond inst_nvars",)),
    (dict(ab=[0, 1, 2, 3]), ("assumption literal beyond inst_nvars",)),     # the empty formula assumes -1
])
def test_ranges_literals_and_assumptions(over, words):
    _refused(*_call(**over), *words)


@pytest.mark.parametrize("bad", [0, I32_MIN])
def test_literals_without_a_variable(bad):
    lits = list(LITS)
    lits[8] = bad
    _refused(*_call(lits=lits), "literal 0 / INT32_MIN")


def test_capacities_room_cap_and_strides():
    _refused(*_call(ccap=0), "non-positive proof capacity")
    _refused(*_call(lcap=-5), "non-positive proof capacity")
    _refused(*_call(ccap=2 ** 31 - 1), "proof capacity beyond the 32-bit offsets")
    _refused(*_call(room_cap=-1), "negative room_cap")
    _refused(*_call(stride=0), "row stride < 1")
    _refused(*_call(stride=5), "row stride < number of variables")
    _refused(*_call(core_stride=-1), "negative core_stride")


def test_past_the_variable_limit_is_too_large_before_any_launch():
    top = _capi.CDCL_SOUND_MAX_VARS + 1
    _refused(*_call(nv=[3, 0, top], al=[3, -1, top], stride=top), f"variable {top} is beyond the layout's {top - 1}",
             code=ERR_TOO_LARGE)


def test_device_forms_refuse_what_they_can_see():
    L = _capi.load()
    p = 4096   # never dereferenced

    def solve(n=1, max_vars=3, mlen=3, stride=3, core_stride=2, ptrs=None):
        q = ptrs or [p] * 15
        return L.satmi_cdcl_assume_batch_device(n, q[0], q[1], q[2], q[3], max_vars, mlen, 0, 0.0, q[4], q[5], q[6],
                                                q[7], q[8], q[9], stride, q[10], q[11], q[12], q[13], q[14],
                                                core_stride, None)

    def packed(n=1, ccap=4, lcap=4, ptrs=None):
        q = ptrs or [p] * 8
        return L.satmi_cdcl_assume_pack_device(n, q[0], q[1], q[2], q[3], q[4], q[5], ccap, q[6], lcap, q[7], None)
    assert solve(n=-1) == ERR_ARG and "satmi_cdcl_assume_batch_device: negative formula count" in L.satmi_last_error().decode()
    assert solve(max_vars=-1) == ERR_ARG and solve(mlen=-1) == ERR_ARG and solve(stride=0) == ERR_ARG
    assert solve(core_stride=-1) == ERR_ARG and "negative core_stride" in L.satmi_last_error().decode()
    assert solve(n=0) == _capi.OK and packed(n=0) == _capi.OK
    assert solve(max_vars=_capi.CDCL_SOUND_MAX_VARS + 1) == ERR_TOO_LARGE
    for null in range(15):
        q = [p] * 15
        q[null] = None
        assert solve(ptrs=q) == ERR_ARG, null
        assert "null pointer" in L.satmi_last_error().decode()
    assert packed(n=-1) == ERR_ARG and packed(ccap=0) == ERR_ARG and packed(lcap=0) == ERR_ARG
    for null in range(8):
        q = [p] * 8
        q[null] = None
        assert packed(ptrs=q) == ERR_ARG, null
        assert "satmi_cdcl_assume_pack_device: null pointer" in L.satmi_last_error().decode()


def test_pack_assumptions():
    begin, lits, top = cdcl_sound.pack_assumptions([[3, -1], [], [-6]], 3)
    assert begin.tolist() == AB and lits.tolist() == [3, -1, -6] and top.tolist() == [3, 0, 6]
    begin, lits, top = cdcl_sound.pack_assumptions(None, 2)
    assert begin.tolist() == [0, 0, 0] and lits.size == 1 and top.tolist() == [0, 0]
    with pytest.raises(ValueError, match="one list"):
        cdcl_sound.pack_assumptions([[1]], 2)
    for bad in (0, I32_MIN, 2 ** 31):
        with pytest.raises(ValueError, match="nonzero"):
            cdcl_sound.pack_assumptions([[bad]], 1)


def test_proof_of_cdcl_assumed_arguments():
    for r in ({"sat": True, "proof": None, "core": None}, {"sat": None, "proof": None, "core": None},
              {"sat": False, "proof": [[]], "core": None}):
        with pytest.raises(ValueError, match="no refutation"):
            proof_of_cdcl_assumed([[1]], r)
    with pytest.raises(ValueError, match="core_stride"):
        proof_of_cdcl_assumed([[1]], {"sat": False, "proof": [[]], "core": [], "core_len": 1})
    assert proof_of_cdcl_assumed([(1, 2)], {"sat": False, "proof": [(2,), ()], "core": [-2, -1]}) == \
        ([[1, 2], [-2], [-1]], [[2], []])
    assert proof_of_cdcl_assumed([[1], [-1]], {"sat": False, "proof": [[]], "core": []}) == ([[1], [-1]], [[]])
