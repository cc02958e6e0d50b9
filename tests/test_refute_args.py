"""CPU checks of satmi_check_refutations_host's refusals through the C ABI, in the
manner of tests/test_host_args.py: both CSR triples go through batch_keys.h before
any HIP call, so every refusal below comes back without a GPU, under the entry
point's name, with the triple and the cause named and the outputs untouched."""
import ctypes

import numpy as np
import pytest

import refute_rows as rr
from satmi import _capi
from satmi.refute import check_refutations, debug_grid

ERR_ARG, ERR_TOO_LARGE = -1, -3
SENTINEL = 77
WHO = "satmi_check_refutations_host"

# three formulas, the middle one empty, and their proofs, the last one empty
ICB, CLB, LITS = [0, 2, 2, 5], [0, 2, 3, 6, 7, 9], [1, -2, 3, -4, 5, 6, 2, -1, -6]
PIB, PCB, PLITS = [0, 2, 3, 3], [0, 1, 1, 3], [3, 1, -2]
B = 3


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i32(x):
    return None if x is None else np.array(x, dtype=np.int64).astype(np.int32)


def _call(count=B, out=True, lemma_ok=True, **over):
    """The host form on the arrays above, those in `over` replaced (None = a NULL pointer)
    -> (return code, message, out, lemma_ok), the outputs pre-filled with SENTINEL."""
    a = {k: _i32(over.get(k, v)) for k, v in
         (("icb", ICB), ("clb", CLB), ("lits", LITS), ("pib", PIB), ("pcb", PCB), ("plits", PLITS))}
    o = np.full(B * _capi.REFUTE_NWORDS, SENTINEL, np.int32)
    ok = np.full(PIB[-1], SENTINEL, np.int32)
    L = _capi.load()
    rc = L.satmi_check_refutations_host(count, _p(a["icb"]), _p(a["clb"]), _p(a["lits"]), _p(a["pib"]), _p(a["pcb"]),
                                        _p(a["plits"]), _p(o) if out else None, _p(ok) if lemma_ok else None)
    msg = L.satmi_last_error()
    return rc, msg.decode() if msg else "", o, ok


def _refused(rc, msg, o, ok, *words, code=ERR_ARG):
    assert rc == code, msg
    assert msg.startswith(WHO + ": ") and all(w in msg for w in words), msg
    assert (o == SENTINEL).all() and (ok == SENTINEL).all()


def test_constants_match_the_header_and_the_evaluator():
    assert (_capi.REFUTE_FAILED, _capi.REFUTE_PROVEN, _capi.REFUTE_OPEN) == (rr.FAILED, rr.PROVEN, rr.OPEN)
    assert (_capi.REFUTE_TAUTOLOGY, _capi.REFUTE_BAD_LITERAL) == (rr.TAUTOLOGY, rr.BAD_LITERAL)
    assert _capi.REFUTE_MAX_VARS == rr.MAX_VARS and _capi.REFUTE_NWORDS == len(_capi.REFUTE_WORDS) == 4
    assert _capi.load().satmi_abi_version() == 2


def test_negative_count():
    _refused(*_call(count=-1), "negative formula count")


def test_empty_batch_is_ok():
    """B = 0 returns SATMI_OK whatever the pointers are, and touches nothing."""
    for kw in ({}, dict(icb=None, clb=None, lits=None, pib=None, pcb=None, plits=None, out=False, lemma_ok=False)):
        rc, _, o, ok = _call(count=0, **kw)
        assert rc == _capi.OK and (o == SENTINEL).all() and (ok == SENTINEL).all()
    assert check_refutations([], []) == []


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
    """SATMI_ERR_TOO_LARGE before any launch, from either triple, either sign; the limit itself
    passes the check (what comes then needs a device: tests/test_refute_gpu.py)."""
    for big in (rr.MAX_VARS + 1, -(rr.MAX_VARS + 1), 2 ** 31 - 1):
        lits = list(LITS if name == "lits" else PLITS)
        lits[at] = big
        _refused(*_call(**{name: lits}), str(abs(big)), str(rr.MAX_VARS), code=ERR_TOO_LARGE)
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        check_refutations([[[1, rr.MAX_VARS + 1]]], [[[1]]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        check_refutations([[[1]]], [[[-(rr.MAX_VARS + 1)]]])


def test_device_form_refuses_what_it_can_see():
    """satmi_check_refutations_device refuses before it touches the device."""
    L = _capi.load()
    p = 4096   # never dereferenced
    for n, mv, mcl, rc in ((-1, 3, 3, ERR_ARG), (1, -1, 3, ERR_ARG), (1, 3, -1, ERR_ARG),
                           (1, rr.MAX_VARS + 1, 3, ERR_TOO_LARGE), (0, 3, 3, _capi.OK)):
        assert L.satmi_check_refutations_device(n, p, p, p, p, p, p, mv, mcl, p, None, None) == rc
    for null in range(7):
        args = [p] * 7
        args[null] = None
        assert L.satmi_check_refutations_device(1, *args[:6], 3, 3, args[6], None, None) == ERR_ARG
        assert "null pointer" in L.satmi_last_error().decode()


def test_python_wrapper_arguments():
    with pytest.raises(ValueError, match="one list of lemmas per formula"):
        check_refutations([[[1]]], [])
    with pytest.raises(ValueError, match="literal 0"):
        check_refutations([[[1]]], [[[0]]])


def test_debug_grid_arguments():
    L = _capi.load()
    for wg, wpg in ((-1, 0), (0, 3), (0, 8), (1, -1), (0, 64)):
        assert L.satmi_refute_debug_grid(wg, wpg) == ERR_ARG
        assert "satmi_refute_debug_grid" in L.satmi_last_error().decode()
        with pytest.raises(_capi.SatmiError):
            debug_grid(wg, wpg)
    for wg, wpg in ((0, 1), (5, 2), (1, 4), (0, 0)):
        debug_grid(wg, wpg)
