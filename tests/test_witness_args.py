"""CPU checks of satmi_witness_models_host's refusals through the C ABI, in the manner
of tests/test_trim_args.py: both CSR triples go through batch_keys.h and the stages
through the entry point's own walk before any HIP call, so every refusal below comes
back without a GPU, under the entry point's own name and with the outputs untouched;
and the two stage builders' ValueErrors."""
import ctypes
import os

import numpy as np
import pytest

import witness_rows as wr
from satmi import _capi
from satmi.witness import (debug_grid, record_of, stages_of_elimination, stages_of_resolution, witness_models)

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_witness_models_host"

# three formulas, the middle one empty, their records, the last one empty, and their stages
ICB, CLB, LITS = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6]
PIB, PCB, PLITS = [0, 2, 3, 3], [0, 1, 1, 3], [3, 1, -2]
ISB, SVAR, SLO, SHI = [0, 2, 2, 4], [1, 3, 6, 2], [0, 2, 0, 3], [4, 2, 3, 3]
B, STRIDE = 3, 6


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i32(x):
    return None if x is None else np.array(x, dtype=np.int64).astype(np.int32)


def _call(count=B, out=True, lens=True, rows=True, highest_only=0, stride=STRIDE, **over):
    """The host form on the arrays above, those in `over` replaced (None = a NULL pointer)
    -> (return code, message, out, row_len, row_lits), the outputs pre-filled with SENTINEL."""
    a = {k: _i32(over.get(k, v)) for k, v in
         (("icb", ICB), ("clb", CLB), ("lits", LITS), ("pib", PIB), ("pcb", PCB), ("plits", PLITS),
          ("isb", ISB), ("svar", SVAR), ("slo", SLO), ("shi", SHI))}
    o = np.full(B * _capi.WITNESS_NWORDS, SENTINEL, np.int32)
    rl = np.full(B, SENTINEL, np.int32)
    rw = np.full(B * STRIDE, SENTINEL, np.int32)
    L = _capi.load()
    rc = L.satmi_witness_models_host(count, *(_p(a[k]) for k in ("icb", "clb", "lits", "pib", "pcb", "plits", "isb",
                                                                 "svar", "slo", "shi")),
                                     highest_only, _p(o) if out else None, _p(rl) if lens else None,
                                     _p(rw) if rows else None, stride)
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o, rl, rw


def _refused(rc, msg, o, rl, rw, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert (o == SENTINEL).all() and (rl == SENTINEL).all() and (rw == SENTINEL).all()


def test_constants_match_the_header_and_the_rows():
    assert _capi.WITNESS_MAX_VARS == _capi.CHECK_MAX_VARS == wr.MAX_VARS == 524287
    assert _capi.WITNESS_NWORDS == len(_capi.WITNESS_WORDS) == wr.NWORDS == 6
    assert (_capi.WITNESS_NOT_MODEL, _capi.WITNESS_MODEL) == (wr.NOT_MODEL, wr.MODEL) == (0, 1)
    assert (_capi.WITNESS_BAD_LITERAL, _capi.WITNESS_BAD_STAGE, _capi.WITNESS_ROW_TRUNCATED) == \
        (wr.BAD_LITERAL, wr.BAD_STAGE, wr.ROW_TRUNCATED) == (1, 2, 4)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "satmi.h")).read()
    for name, value in (("NWORDS", 6), ("NOT_MODEL", 0), ("MODEL", 1), ("BAD_LITERAL", 1), ("BAD_STAGE", 2),
                        ("ROW_TRUNCATED", 4), ("MAX_VARS", 524287)):
        assert f"#define SATMI_WITNESS_{name} {value} " in text, name
    assert _capi.load().satmi_abi_version() == 2


def test_the_arrays_above_pass_every_check_the_rule_knows():
    """(what comes then needs a device: tests/test_witness_gpu.py)"""
    for b in range(B):
        m, p = ICB[b + 1] - ICB[b], PIB[b + 1] - PIB[b]
        for t in range(ISB[b], ISB[b + 1]):
            assert 1 <= SVAR[t] <= 6 and 0 <= SLO[t] <= SHI[t] <= m + p


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_own_arguments():
    _refused(*_call(stride=0), "stride < 1")
    _refused(*_call(stride=-3), "stride < 1")
    _refused(*_call(highest_only=2), "highest_only is 0 or 1")
    _refused(*_call(highest_only=-1), "highest_only is 0 or 1")


def test_empty_batch_is_ok():
    """B = 0 returns SATMI_OK whatever the pointers are, and touches nothing."""
    for kw in ({}, dict(icb=None, clb=None, lits=None, pib=None, pcb=None, plits=None, isb=None, svar=None, slo=None,
                        shi=None, out=False, lens=False, rows=False)):
        rc, _, o, rl, rw = _call(count=0, **kw)
        assert rc == _capi.OK and (o == SENTINEL).all() and (rl == SENTINEL).all() and (rw == SENTINEL).all()
    assert witness_models([], [], []) == []


@pytest.mark.parametrize("name,triple", [("icb", "formulas"), ("clb", "formulas"), ("lits", "formulas"),
                                         ("pib", "records"), ("pcb", "records"), ("plits", "records"),
                                         ("isb", "stages"), ("svar", "stages"), ("slo", "stages"),
                                         ("shi", "stages")])
def test_null_input_pointers(name, triple):
    _refused(*_call(**{name: None}), triple, "null pointer")


@pytest.mark.parametrize("which", ["out", "lens", "rows"])
def test_null_output_pointers(which):
    _refused(*_call(**{which: False}), "null pointer")


@pytest.mark.parametrize("over,words", [
    (dict(icb=[0, 2, 1, 5]), ("formulas", "clause ranges are not ascending")),
    (dict(icb=[-1, 2, 2, 5]), ("formulas", "clause ranges are not ascending")),
    (dict(clb=[0, 2, 1, 6, 7, 9]), ("formulas", "literal ranges are not ascending")),
    (dict(clb=[-1, 2, 3, 6, 7, 9]), ("formulas", "literal ranges are not ascending")),
    (dict(pib=[0, 2, 1, 3]), ("records", "clause ranges are not ascending")),
    (dict(pib=[-1, 2, 3, 3]), ("records", "clause ranges are not ascending")),
    (dict(pcb=[0, 2, 1, 3]), ("records", "literal ranges are not ascending")),
    (dict(pcb=[-2, 1, 1, 3]), ("records", "literal ranges are not ascending")),
    (dict(isb=[0, 2, 1, 4]), ("stages", "stage ranges are not ascending")),
    (dict(isb=[-1, 2, 2, 4]), ("stages", "stage ranges are not ascending")),
    (dict(isb=[0, 3, 2, 4]), ("stages", "stage ranges are not ascending")),
])
def test_ranges_that_do_not_ascend(over, words):
    _refused(*_call(**over), *words)


@pytest.mark.parametrize("bad", [0, wr.I32_MIN])
@pytest.mark.parametrize("name,at,triple", [("lits", 0, "formulas"), ("lits", 8, "formulas"),
                                            ("plits", 0, "records"), ("plits", 2, "records")])
def test_literals_without_a_variable(name, at, triple, bad):
    lits = list(LITS if name == "lits" else PLITS)
    lits[at] = bad
    _refused(*_call(**{name: lits}), triple, "literal 0 / INT32_MIN")


@pytest.mark.parametrize("at,var", [(0, 0), (1, -3), (2, 7), (3, wr.I32_MIN), (0, 2 ** 31 - 1)])
def test_stage_variable_outside_the_batch(at, var):
    """max_vars is 6 here, computed over formulas and records: a stage of variable 7 is refused."""
    svar = list(SVAR)
    svar[at] = var
    _refused(*_call(svar=svar), "stages", "stage variable outside 1 .. max_vars")


@pytest.mark.parametrize("at,lo,hi", [(0, -1, 4), (0, 0, 5), (0, 3, 2), (1, 5, 5), (2, 0, 4), (3, 4, 3),
                                      (3, 0, 2 ** 31 - 1), (2, wr.I32_MIN, 0)])
def test_stage_range_outside_the_instance(at, lo, hi):
    """Instance 0 has m + P = 2 + 2 clauses, instance 2 has 3 + 0: hi may equal that, no more."""
    slo, shi = list(SLO), list(SHI)
    slo[at], shi[at] = lo, hi
    _refused(*_call(slo=slo, shi=shi), "stages", "clause range outside 0 <= lo <= hi <= m + P")


@pytest.mark.parametrize("name,at", [("lits", 4), ("plits", 1)])
def test_variable_beyond_the_limit(name, at):
    """SATMI_ERR_TOO_LARGE at 524,288 variables before any launch, from either triple, either sign."""
    for big in (wr.MAX_VARS + 1, -(wr.MAX_VARS + 1), 2 ** 31 - 1):
        lits = list(LITS if name == "lits" else PLITS)
        lits[at] = big
        _refused(*_call(**{name: lits}), str(abs(big)), str(wr.MAX_VARS), code=ERR_TOO_LARGE)
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        witness_models([[[1, wr.MAX_VARS + 1]]], [[]], [[(1, 0, 1)]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        witness_models([[[1]]], [[[-(wr.MAX_VARS + 1)]]], [[]])


def test_device_form_refuses_what_it_can_see():
    L = _capi.load()
    p = 4096   # never dereferenced
    for n, ho, mv, mcl, stride, rc in ((-1, 0, 3, 3, 1, ERR_ARG), (1, 0, -1, 3, 1, ERR_ARG), (1, 0, 3, -1, 1, ERR_ARG),
                                       (1, 0, 3, 3, 0, ERR_ARG), (1, 2, 3, 3, 1, ERR_ARG),
                                       (1, 0, wr.MAX_VARS + 1, 3, 1, ERR_TOO_LARGE), (0, 1, 3, 3, 1, _capi.OK)):
        assert L.satmi_witness_models_device(n, *[p] * 10, ho, mv, mcl, p, p, p, stride, None) == rc
    assert "satmi_witness_models_device" in L.satmi_last_error().decode()
    for null in range(13):
        args = [p] * 13
        args[null] = None
        assert L.satmi_witness_models_device(1, *args[:10], 0, 3, 3, *args[10:], 1, None) == ERR_ARG
        assert "null pointer" in L.satmi_last_error().decode()


def test_python_wrapper_arguments():
    with pytest.raises(ValueError, match="one list of clauses per formula"):
        witness_models([[[1]]], [], [[]])
    with pytest.raises(ValueError, match="one list per formula"):
        witness_models([[[1]]], [[]], [])
    with pytest.raises(ValueError, match="int32"):
        witness_models([[[1]]], [[]], [[(2 ** 31, 0, 1)]])


def test_debug_grid_arguments():
    L = _capi.load()
    for wg, wpg in ((-1, 0), (0, 3), (0, 8), (1, -1), (0, 64)):
        assert L.satmi_witness_debug_grid(wg, wpg) == ERR_ARG
        assert "satmi_witness_debug_grid" in L.satmi_last_error().decode()
        with pytest.raises(_capi.SatmiError):
            debug_grid(wg, wpg)
    for wg, wpg in ((0, 1), (5, 2), (1, 4), (0, 0)):
        debug_grid(wg, wpg)


@pytest.mark.parametrize("build", [stages_of_elimination, stages_of_resolution])
def test_builders_want_a_record_of_a_true_answer(build):
    f = [[1, 2], [-1]]
    with pytest.raises(ValueError, match="no record"):
        build(f, {"result": 1, "vars": [1, 2], "steps": 2})
    for result in (0, -1, -2):
        with pytest.raises(ValueError, match="not 1"):
            build(f, {"result": result, "vars": [1], "steps": 1, "clauses": [[[2]]]})
    with pytest.raises(ValueError, match="no record"):
        record_of({"result": 1})


def test_builders_number_the_record_as_the_rule_does():
    """The builders against the restatement's own (tests/witness_rows.py), on its records."""
    for f in wr.random_formulas(3, 60, True) + wr.random_formulas(4, 60, False):
        ok, popped, lists = wr.ref_davis_putnam(f)
        if ok:
            r = {"result": 1, "vars": popped, "steps": len(popped), "clauses": lists}
            assert stages_of_elimination(f, r) == wr.elimination_stages(len(f), popped, lists)
            assert record_of(r) == [c for group in lists for c in group]
        ok, rec = wr.ref_resolution(f)
        if ok:
            r = {"result": 1, "passes": 2, "clauses": [rec[:1], rec[1:]]}
            assert stages_of_resolution(f, r) == wr.resolution_stages(f, rec)
            assert record_of(r) == rec
    assert stages_of_elimination([[1, 2], [-1]], {"result": 1, "vars": [2, 1], "clauses": [[[-1]], []]}) == \
        [(1, 2, 3), (2, 0, 2)]
    assert stages_of_resolution([[1, 3]], {"result": 1, "clauses": [[[-3, 5]]]}) == [(1, 0, 2), (3, 0, 2), (5, 0, 2)]
