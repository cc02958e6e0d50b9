"""What the wrappers share on the way into libsatmi.so: ctypes pointers (all of
them), and for resolution and Davis-Putnam a formula's CSR arrays and a
batched call's packed input."""
import ctypes
import itertools

import numpy as np

from . import _capi


def _csr(formula):
    """The formula's CSR host arrays (clause offsets, literals), built without a
    per-literal Python loop (a call's conversion is part of its time)."""
    off = np.zeros(len(formula) + 1, dtype=np.int32)
    np.cumsum(np.fromiter(map(len, formula), dtype=np.int32, count=len(formula)), out=off[1:])
    n = int(off[-1])
    if n == 0:
        return off, np.zeros(1, dtype=np.int32)
    # (a literal outside int32 raises OverflowError here, like np.asarray did)
    flat = np.fromiter(itertools.chain.from_iterable(formula), dtype=np.int32, count=n)
    if not flat.all():
        raise ValueError("literal 0 is not allowed (REF.py:51)")
    return off, flat


def _p(a, t=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(t))


def packed(formulas):
    """`formulas` (a list of formulas or a cnf.CnfBatch) -> (the CnfBatch, its three
    CSR arrays as contiguous int32) and a GPU is required, or None for an empty batch."""
    from . import cnf
    if isinstance(formulas, cnf.CnfBatch):
        cb = formulas
    else:
        formulas = list(formulas)
        cb = cnf.pack(formulas) if formulas else None
    if cb is None or cb.num_instances == 0:
        return None
    _capi.require_gpu()
    return cb, tuple(np.ascontiguousarray(a, dtype=np.int32)
                     for a in (cb.inst_clause_begin, cb.clause_lit_begin, cb.lits))

