"""CPU checks of satmi_trim_refutations_host's refusals through the C ABI, in the
manner of tests/test_refute_args.py: both CSR triples go through batch_keys.h
before any HIP call, so every refusal below comes back without a GPU, under the
entry point's own name, with the forward check's messages and the outputs
untouched."""
import ctypes

import numpy as np
import pytest

import refute_rows as rr
import trim_rows as tr
from satmi import _capi
from satmi.refute import trim_debug_grid, trim_refutations

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_trim_refutations_host"

# three formulas, the middle one empty, and their proofs, the last one empty
ICB, CLB, LITS = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6]
PIB, PCB, PLITS = [0, 2, 3, 3], [0, 1, 1, 3], [3, 1, -2]
B = 3


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i32(x):
    return None if x is None else np.array(x, dtype=np.int64).astype(np.int32)


def _call(count=B, out=True, core=True, lemma=True, **over):
    """The host form on the arrays above, those in `over` replaced (None = a NULL pointer)
    -> (return code, message, out, core, lemma), the outputs pre-filled with SENTINEL."""
    a = {k: _i32(over.get(k, v)) for k, v in
         (("icb", ICB), ("clb", CLB), ("lits", LITS), ("pib", PIB), ("pcb", PCB), ("plits", PLITS))}
    o = np.full(B * _capi.TRIM_NWORDS, SENTINEL, np.int32)
    co = np.full(ICB[-1], SENTINEL, np.int32)
    le = np.full(PIB[-1], SENTINEL, np.int32)
    L = _capi.load()
    rc = L.satmi_trim_refutations_host(count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["pib"]), _p(a["pcb"]),
                                       _p(a["plits"]), _p(o) if out else None, _p(co) if core else None,
                                       _p(le) if lemma else None)
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o, co, le


def _refused(rc, msg, o, co, le, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert (o == SENTINEL).all() and (co == SENTINEL).all() and (le == SENTINEL).all()


def test_constants_match_the_header_and_the_rows():
    assert _capi.TRIM_MAX_VARS == tr.MAX_VARS == 16383
    assert _capi.TRIM_NWORDS == len(_capi.TRIM_WORDS) == tr.NWORDS == 6
    assert _capi.TRIM_WORDS[:4] == _capi.REFUTE_WORDS
    assert _capi.load().satmi_abi_version() == 2


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_empty_batch_is_ok():
    """B = 0 returns SATMI_OK whatever the pointers are, and touches nothing."""
    for kw in ({}, dict(icb=None, clb=None, lits=None, pib=None, pcb=None, plits=None, out=False, core=False,
                        lemma=False)):
        rc, _, o, co, le = _call(count=0, **kw)
        assert rc == _capi.OK and (o == SENTINEL).all() and (co == SENTINEL).all() and (le == SENTINEL).all()
    assert trim_refutations([], []) == []


@pytest.mark.parametrize("name,triple", [("icb", "formulas"), ("clb", "formulas"), ("lits", "formulas"),
                                         ("pib", "proofs"), ("pcb", "proofs"), ("plits", "proofs")])
def test_null_input_pointers(name, triple):
    _refused(*_call(**{name: None}), triple, "null pointer")


def test_null_output_pointer():
    _refused(*_call(out=False), "null pointer")


@pytest.mark.parametrize("over,words", [
    (dict(icb=[0, 2, 1, 5]), ("formulas", "clause ranges are not ascending")),
    (dict(icb=[-1, 2, 2, 5]), ("formulas", "clause ranges are not ascending")),
    (dict(clb=[0, 2, 1, 6, 7, 9]), ("formulas", "literal ranges are not ascending")),
    (dict(clb=[-1, 2, 3, 6, 7, 9]), ("formulas", "literal ranges are not ascending")),
    (dict(pib=[0, 2, 1, 3]), ("proofs", "clause ranges are not ascending")),
    (dict(pib=[-1, 2, 3, 3]), ("proofs", "clause ranges are not ascending")),
    (dict(pcb=[0, 2, 1, 3]), ("proofs", "literal ranges are not ascending")),
    (dict(pcb=[-2, 1, 1, 3]), ("proofs", "literal ranges are not ascending")),
])
def test_ranges_that_do_not_ascend(over, words):
    _refused(*_call(**over), *words)


@pytest.mark.parametrize("bad", [0, rr.I32_MIN])
@pytest.mark.parametrize("name,at,triple", [("lits", 0, "formulas"), ("lits", 8, "formulas"),
                                            ("plits", 0, "proofs"), ("plits", 2, "proofs")])
def test_literals_without_a_variable(name, at, triple, bad):
    lits = list(LITS if name == "lits" else PLITS)
    lits[at] = bad
    _refused(*_call(**{name: lits}), triple, "literal 0 / INT32_MIN")


@pytest.mark.parametrize("name,at", [("lits", 4), ("plits", 1)])
def test_variable_beyond_the_limit(name, at):
    """SATMI_ERR_TOO_LARGE at 16,384 variables before any launch, from either triple, either
    sign (the limit itself passes the check; what comes then needs a device: tests/test_trim_gpu.py)."""
    for big in (tr.MAX_VARS + 1, -(tr.MAX_VARS + 1), rr.MAX_VARS, 2 ** 31 - 1):
        lits = list(LITS if name == "lits" else PLITS)
        lits[at] = big
        _refused(*_call(**{name: lits}), str(abs(big)), str(tr.MAX_VARS), code=ERR_TOO_LARGE)
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        trim_refutations([[[1, tr.MAX_VARS + 1]]], [[[1]]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        trim_refutations([[[1]]], [[[-(tr.MAX_VARS + 1)]]])


def test_device_form_refuses_what_it_can_see():
    """satmi_trim_refutations_device refuses before it touches the device; the two mark arrays
    are the walk's own state, so it needs both."""
    L = _capi.load()
    p = 4096   # never dereferenced
    for n, mv, mcl, rc in ((-1, 3, 3, ERR_ARG), (1, -1, 3, ERR_ARG), (1, 3, -1, ERR_ARG),
                           (1, tr.MAX_VARS + 1, 3, ERR_TOO_LARGE), (0, 3, 3, _capi.OK)):
        assert L.satmi_trim_refutations_device(n, p, p, p, p, p, p, mv, mcl, p, p, p, None) == rc
    assert "satmi_trim_refutations_device" in L.satmi_last_error().decode()
    for null in range(9):
        args = [p] * 9
        args[null] = None
        assert L.satmi_trim_refutations_device(1, *args[:6], 3, 3, *args[6:], None) == ERR_ARG
        assert "null pointer" in L.satmi_last_error().decode()


def test_debug_grid_arguments():
    L = _capi.load()
    for wg, wpg in ((-1, 0), (0, 3), (0, 8), (1, -1), (0, 64)):
        assert L.satmi_trim_debug_grid(wg, wpg) == ERR_ARG
        assert "satmi_trim_debug_grid" in L.satmi_last_error().decode()
        with pytest.raises(_capi.SatmiError):
            trim_debug_grid(wg, wpg)
    for wg, wpg in ((0, 1), (5, 2), (1, 4), (0, 0)):
        trim_debug_grid(wg, wpg)
