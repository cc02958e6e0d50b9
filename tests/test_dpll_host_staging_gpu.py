"""GPU: satmi_dpll_batch_host's staging (csrc/dpll.hip) -- the blocks it carves
out of its one allocation, what it copies in and what it copies back -- called
directly, once per kernel class, on a batch of three tiny formulas one of which
has no clauses; every status, counter, model and root literal against the oracle.

The calls differ in what the staging turns on: a caller's assignment or none,
sol_cap = 0 with no solution and no root outputs wanted, and a batch without a
single literal under assignments without a single entry (the blocks that are
sized max(..., 1))."""
import ctypes
import random

import numpy as np
import pytest

import oracle
from satmi import _capi, cnf

pytestmark = pytest.mark.gpu

CTR = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")


def _formulas():
    rng = random.Random(31)

    def clause(n, k):
        return [v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), k)]
    return [[clause(12, 3) for _ in range(40)], [], [clause(8, rng.randint(1, 3)) for _ in range(20)]]


def _ptr(a, t=ctypes.c_int32):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def _batch_host(fs, mode, inits, max_solutions, sol_cap, want_roots):
    """satmi_dpll_batch_host as a C caller would call it: sol_cap = 0 passes no
    solution buffers, want_roots = False no root buffers."""
    L = _capi.load()
    batch = cnf.pack(fs)
    B = len(fs)
    stride = max([1, int(batch.inst_nvars.max(initial=0))] + [abs(x) for a in inits or [] for x in a])
    init_begin = init_lits = None
    if inits is not None:
        init_begin = np.cumsum([0] + [len(a) for a in inits]).astype(np.int32)
        init_lits = np.array([x for a in inits for x in a], dtype=np.int32)   # may have no entry at all
    status = np.full(B, -9, dtype=np.int32)
    counters = np.full((B, _capi.NCOUNTERS), -9, dtype=np.int64)
    sol_len = np.full((B, sol_cap), -9, dtype=np.int32) if sol_cap else None
    sol_lits = np.full((B, sol_cap, stride), -9, dtype=np.int32) if sol_cap else None
    root_len = np.full(B, -9, dtype=np.int32) if want_roots else None
    root_lits = np.full((B, stride), -9, dtype=np.int32) if want_roots else None
    rc = L.satmi_dpll_batch_host(
        B, _ptr(batch.inst_clause_begin), _ptr(batch.clause_lit_begin), _ptr(batch.lits), _ptr(batch.inst_nvars),
        _ptr(init_begin), _ptr(init_lits), mode, max_solutions, 0, 0.0, sol_cap, stride, _ptr(status),
        _ptr(counters, ctypes.c_int64), _ptr(sol_len), _ptr(sol_lits), _ptr(root_len), _ptr(root_lits))
    _capi.check(rc, "satmi_dpll_batch_host")
    return status, counters, sol_len, sol_lits, root_len, root_lits


# kernel class: (policy, the kernel it must plan, mode, inits, max_solutions, sol_cap, want_roots)
CALLS = {
    "general": (_capi.KERNEL_GENERAL, _capi.KERNEL_GENERAL, "ref", [[1, -2], [], [9, 3]], 0, 16, True),
    # (REF mode: under SOUND without a dict the WIDE policy still leaves eligible batches to the clause kernels)
    "wide": (_capi.KERNEL_WIDE, _capi.KERNEL_WIDE, "ref", None, 0, 0, False),
    "clause": (_capi.KERNEL_AUTO, _capi.KERNEL_INC, "sound", None, 1, 1, True),
    "no_literals": (_capi.KERNEL_AUTO, _capi.KERNEL_GENERAL, "sound", [[], [], []], 0, 2, True),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_batch_host_stages_every_block(name):
    policy, kernel, mode, inits, max_solutions, sol_cap, want_roots = CALLS[name]
    fs = [[], [], []] if name == "no_literals" else _formulas()
    assert any(not f for f in fs) and all(len(f) <= 60 for f in fs)
    m = {"ref": _capi.MODE_REF, "sound": _capi.MODE_SOUND}[mode]
    lens = [len(c) for f in fs for c in f]
    shape = (max([max(abs(l) for c in f for l in c) for f in fs if f] + [0]), max(len(f) for f in fs),
             max(sum(len(c) for c in f) for f in fs), max(lens + [0]))
    _capi.set_kernel(policy)
    try:
        assert _capi.plan(*shape, mode=m, has_init=inits is not None)[0] == kernel
        status, counters, sol_len, sol_lits, root_len, root_lits = _batch_host(fs, m, inits, max_solutions, sol_cap,
                                                                               want_roots)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    for b, f in enumerate(fs):
        o = oracle.dpll(f, mode, max_solutions=max_solutions, init=inits[b] if inits else None, sol_cap=max(sol_cap, 1))
        print(name, b, int(status[b]), counters[b].tolist(), o["status"], o["counters"])
        assert int(status[b]) == o["status"], (name, b)
        assert [int(counters[b, i]) for i in range(len(CTR))] == [o["counters"][k] for k in CTR], (name, b)
        if sol_cap:
            k = min(o["counters"]["solutions"], sol_cap)
            assert [sol_lits[b, s, :sol_len[b, s]].tolist() for s in range(k)] == o["solutions"][:k], (name, b)
        if want_roots:
            assert root_lits[b, :root_len[b]].tolist() == o["root_assign"], (name, b)
