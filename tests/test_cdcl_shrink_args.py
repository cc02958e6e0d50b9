"""CPU checks of satmi_cdcl_shrink_batch_host's refusals through the C ABI, in the manner of
tests/test_cdcl_carry_args.py: the host form makes satmi_cdcl_carry_batch_host's checks, and
asks for h_shrink_info, before any HIP call, so every refusal below comes back without a GPU,
under the entry point's name, with the cause named and the outputs untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

from satmi import _capi

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_cdcl_shrink_batch_host"
I32_MIN = -(2 ** 31)

# three formulas, the middle one empty; the first assumes two literals, the last one; the first
# carries two clauses, the last one
ICB, CLB, LITS, NV = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6], [3, 0, 6]
AB, AL = [0, 2, 2, 3], [3, -1, 6]
CIB, CCB, CL = [0, 2, 2, 3], [0, 1, 3, 6], [-3, 1, 2, 6, -4, 5]
B, STRIDE, CCAP, LCAP, CSTRIDE, KCCAP, KLCAP = 3, 6, 8, 16, 2, 8, 16
INPUTS = ("icb", "clb", "lits", "nv", "ab", "al", "cib", "ccb", "cl")
CARRY = ("cib", "ccb", "cl")
KEPT = ("kib", "kcb", "klits")
OUTPUTS = ("status", "counters", "row_len", "row_lits", "pib", "pcb", "plits", "info", "totals", "core_len",
           "core_lits") + KEPT + ("shrink",)
I64 = ("counters", "info", "totals", "shrink")


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_int32))


def _call(count=B, ccap=CCAP, lcap=LCAP, room_cap=0, stride=STRIDE, core_stride=CSTRIDE, kccap=KCCAP, klcap=KLCAP,
          null=(), **over):
    """The host form on the arrays above, those in `over` replaced and those named in `null`
    passed as NULL -> (return code, message, outputs), the outputs pre-filled with SENTINEL."""
    a = dict(zip(INPUTS, (ICB, CLB, LITS, NV, AB, AL, CIB, CCB, CL)))
    a.update(over)
    a = {k: None if k in null else np.array(v, dtype=np.int64).astype(np.int32) for k, v in a.items()}
    sizes = dict(status=B, counters=B * 8, row_len=B, row_lits=B * 8192, pib=B + 1, pcb=CCAP + 1, plits=LCAP,
                 info=B * _capi.CDCL_SOUND_NWORDS, totals=4, core_len=B, core_lits=B * 8, kib=B + 1, kcb=KCCAP + 1,
                 klits=KLCAP, shrink=B * _capi.CDCL_SHRINK_NWORDS)
    o = {k: np.full(n, SENTINEL, np.int64 if k in I64 else np.int32) for k, n in sizes.items()}
    q = {k: None if k in null else v for k, v in o.items()}
    L = _capi.load()
    rc = L.satmi_cdcl_shrink_batch_host(
        count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["nv"]), 0, 0.0, room_cap, _p(q["status"]),
        _p(q["counters"]), _p(q["row_len"]), _p(q["row_lits"]), stride, _p(q["pib"]), _p(q["pcb"]), ccap,
        _p(q["plits"]), lcap, _p(q["info"]), _p(q["totals"]), _p(a["ab"]), _p(a["al"]), _p(q["core_len"]),
        _p(q["core_lits"]), core_stride, _p(a["cib"]), _p(a["ccb"]), _p(a["cl"]), _p(q["kib"]), _p(q["kcb"]), kccap,
        _p(q["klits"]), klcap, _p(q["shrink"]))
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o


def _refused(rc, msg, o, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert all((v == SENTINEL).all() for v in o.values())


# a refusal that only comes after every other check: what lets "accepted up to the first HIP
# call" be seen without a GPU
TOP = _capi.CDCL_SOUND_MAX_VARS + 1
LAST = dict(nv=[3, 0, TOP], stride=TOP)


def _accepted(**kw):
    _refused(*_call(**LAST, **kw), f"variable {TOP} is beyond the layout's {TOP - 1}", code=ERR_TOO_LARGE)


def test_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "satmi.h")).read()
    defs = dict(re.findall(r"#define (SATMI_[A-Z_]+) (\d+)", text))
    assert int(defs["SATMI_CDCL_SHRINK_NWORDS"]) == _capi.CDCL_SHRINK_NWORDS == len(_capi.CDCL_SHRINK_WORDS) == 6
    assert int(defs["SATMI_ABI_VERSION"]) == 2 and _capi.load().satmi_abi_version() == 2
    for name in ("satmi_cdcl_shrink_batch_device", "satmi_cdcl_shrink_batch_host"):
        assert name in _capi.EXPORTED and re.search(r"\bint " + name + r"\(", text)


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_empty_batch_is_ok():
    for null in ((), INPUTS + OUTPUTS):
        rc, _, o = _call(count=0, null=null)
        assert rc == _capi.OK and all((v == SENTINEL).all() for v in o.values())


@pytest.mark.parametrize("name", [n for n in INPUTS if n not in CARRY])
def test_null_input_pointers(name):
    _refused(*_call(null=(name,)), "null pointer")


@pytest.mark.parametrize("name", [n for n in OUTPUTS if n != "info"])
def test_null_output_pointers(name):
    """(h_shrink_info among them, and a kept array alone: the three are there together or not at all)"""
    _refused(*_call(null=(name,)), "null pointer")


@pytest.mark.parametrize("null", [("cib",), ("ccb",), ("cl",), ("cib", "ccb"), ("cib", "cl"), ("ccb", "cl")])
def test_a_carry_triple_with_some_pointers_missing(null):
    _refused(*_call(null=null), "null pointer")


def test_null_carry_and_null_kept_arrays_are_accepted_up_to_the_first_hip_call():
    _accepted()
    _accepted(null=("info",))
    _accepted(null=CARRY)
    _accepted(null=KEPT, kccap=0, klcap=0)
    _accepted(null=CARRY + KEPT, kccap=0, klcap=0)
    _accepted(kccap=0, klcap=0)
    _accepted(core_stride=0, null=("core_lits",))             # the refinement does not read core_lits
    _accepted(null=("cl",), cib=[0, 0, 0, 0], ccb=[0])
    _accepted(cib=[1, 2, 2, 3])
    _refused(*_call(null=KEPT, kccap=1, klcap=0), "null pointer")
    _refused(*_call(null=KEPT, kccap=0, klcap=1), "null pointer")
    _refused(*_call(null=("shrink",), **LAST), "null pointer")        # before the layout's verdict


@pytest.mark.parametrize("over,words", [
    (dict(cib=[-1, 2, 2, 3]), ("carry clause ranges are not ascending",)),
    (dict(cib=[0, 2, 1, 3]), ("carry clause ranges are not ascending",)),
    (dict(cib=[0, 3, 3, 2]), ("carry clause ranges are not ascending",)),
    (dict(ccb=[-1, 1, 3, 6]), ("carry literal ranges are not ascending",)),
    (dict(ccb=[0, 3, 1, 6]), ("carry literal ranges are not ascending",)),
    (dict(ccb=[0, 1, 1, 6]), ("empty carried clause",)),
    (dict(ccb=[0, 0, 3, 6]), ("empty carried clause",)),
    (dict(ccb=[0, 1, 6, 6]), ("empty carried clause",)),
    (dict(cl=[-3, 0, 2, 6, -4, 5]), ("carried literal 0 / INT32_MIN",)),
    (dict(cl=[-3, 1, 2, 6, -4, I32_MIN]), ("carried literal 0 / INT32_MIN",)),
    (dict(cl=[4, 1, 2, 6, -4, 5]), ("carried literal beyond inst_nvars",)),
    (dict(cl=[-3, 1, 2, 6, -4, -7]), ("carried literal beyond inst_nvars",)),
    (dict(cib=[0, 1, 2, 3]), ("carried literal beyond inst_nvars",)),
    (dict(ab=[-1, 2, 2, 3]), ("assumption ranges are not ascending",)),
    (dict(ab=[0, 2, 1, 3]), ("assumption ranges are not ascending",)),
    (dict(al=[3, 0, 6]), ("assumption literal 0 / INT32_MIN",)),
    (dict(al=[3, I32_MIN, 6]), ("assumption literal 0 / INT32_MIN",)),
    (dict(al=[4, -1, 6]), ("assumption literal beyond inst_nvars",)),
    (dict(icb=[0, 2, 1, 5]), ("clause ranges are not ascending",)),
    (dict(nv=[3, -1, 6]), ("negative inst_nvars",)),
    (dict(nv=[3, 0, 5]), ("literal beyond inst_nvars",)),
])
def test_ranges_literals_assumptions_and_carries(over, words):
    _refused(*_call(**over), *words)


def test_capacities_room_cap_and_strides():
    _refused(*_call(ccap=0), "non-positive proof capacity")
    _refused(*_call(lcap=-5), "non-positive proof capacity")
    _refused(*_call(ccap=2 ** 31 - 1), "proof capacity beyond the 32-bit offsets")
    _refused(*_call(room_cap=-1), "negative room_cap")
    _refused(*_call(stride=0), "row stride < 1")
    _refused(*_call(stride=5), "row stride < number of variables")
    _refused(*_call(core_stride=-1), "negative core_stride")
    _refused(*_call(kccap=-1), "negative kept capacity")
    _refused(*_call(klcap=-1), "negative kept capacity")
    _refused(*_call(kccap=2 ** 31 - 1), "kept capacity beyond the 32-bit offsets")
    _refused(*_call(klcap=2 ** 31), "kept capacity beyond the 32-bit offsets")


def test_device_form_refuses_what_it_can_see():
    L = _capi.load()
    p = 4096   # never dereferenced

    def solve(n=1, max_vars=3, mlen=3, stride=3, core_stride=2, ptrs=None):
        q = ptrs or [p] * 19
        return L.satmi_cdcl_shrink_batch_device(n, q[0], q[1], q[2], q[3], max_vars, mlen, 0, 0.0, q[4], q[5], q[6],
                                                q[7], q[8], q[9], stride, q[10], q[11], q[12], q[13], q[14],
                                                core_stride, q[15], q[16], q[17], q[18], None)
    assert solve(n=-1) == ERR_ARG
    assert "satmi_cdcl_shrink_batch_device: negative formula count" in L.satmi_last_error().decode()
    assert solve(max_vars=-1) == ERR_ARG and solve(mlen=-1) == ERR_ARG and solve(stride=0) == ERR_ARG
    assert solve(core_stride=-1) == ERR_ARG and "negative core_stride" in L.satmi_last_error().decode()
    assert solve(n=0) == _capi.OK
    assert solve(max_vars=_capi.CDCL_SOUND_MAX_VARS + 1) == ERR_TOO_LARGE
    for null in range(19):
        if null == 15:      # carry_in may be NULL: nothing carried
            continue
        q = [p] * 19
        q[null] = None
        assert solve(ptrs=q) == ERR_ARG, null
        assert "satmi_cdcl_shrink_batch_device: null pointer" in L.satmi_last_error().decode()
    q = [p] * 19
    q[14] = None        # no core_lits with core_stride 0: past the argument checks
    assert solve(core_stride=0, max_vars=_capi.CDCL_SOUND_MAX_VARS + 1, ptrs=q) == ERR_TOO_LARGE


def test_incremental_solver_and_solve_take_the_keyword():
    import inspect
    from satmi import incremental, solvers
    assert inspect.signature(incremental.Solver.solve).parameters["minimal_core"].default is False
    assert inspect.signature(solvers.cdcl_sound_solve).parameters["minimal_core"].default is False
    with incremental.Solver(bootstrap_with=[[1, 2]]) as s:
        assert s.accum_stats() == {"conflicts": 0, "decisions": 0, "propagated": 0, "rounds": 0, "queries": 0}
