"""The host arithmetic of the DPLL entry points (csrc/dpll.hip: the two storage
layouts of the general kernel and the choice of kernel; csrc/dpll_scan.hip:
the clause kernels' eligibility layout), asked through the three queries that
make no HIP call, so the answers are the same with and without a GPU:

    satmi_dpll_lds_bytes, satmi_dpll_scan_lds_bytes, and satmi_dpll_plan
    wherever it cannot answer with a clause kernel (REF mode, a caller's
    assignment, the GENERAL policy): that answer asks the runtime for occupancy.

`queries(L)` lists the questions, on the edges of the layouts and of the
choice; `ask(L, q)` answers one.  tests/golden/make_golden_plan.py records the
answers of one build in tests/golden/dpll_plan_table.json, and
tests/test_dpll_plan_table.py holds every later build to them.
"""
import ctypes
import random

from satmi import _capi

A, G, S, I, W = (_capi.KERNEL_AUTO, _capi.KERNEL_GENERAL, _capi.KERNEL_SCAN, _capi.KERNEL_INC, _capi.KERNEL_WIDE)
REF, SOUND = _capi.MODE_REF, _capi.MODE_SOUND

# (policy, mode, has_init) under which satmi_dpll_plan never answers with a
# clause kernel.  A pinned SCAN / INC policy that the call does not fit plans
# the general kernel (only a launch rejects it).
NO_CLAUSE_KERNEL = ((A, REF, 0), (A, SOUND, 1), (G, SOUND, 0), (W, REF, 0), (G, REF, 1), (W, SOUND, 1), (I, REF, 0),
                    (S, SOUND, 1))


def ask(L, q):
    """The library's answer to the query `q` (a dict of its inputs)."""
    v, c, l, k = q["shape"]
    if q["fn"] == "lds_bytes":
        return {"bytes": L.satmi_dpll_lds_bytes(v, c, l)}
    if q["fn"] == "scan_lds_bytes":
        return {"bytes": L.satmi_dpll_scan_lds_bytes(v, c, l, k)}
    kern, lds, waves = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_int(0)
    L.satmi_dpll_set_kernel(q["policy"])
    try:
        rc = L.satmi_dpll_plan(v, c, l, k, q["mode"], q["has_init"], ctypes.byref(kern), ctypes.byref(lds),
                               ctypes.byref(waves))
    finally:
        L.satmi_dpll_set_kernel(A)
    return {"rc": rc, "kernel": kern.value, "lds_bytes_per_wave": lds.value, "waves_per_cu": waves.value}


def _last_true(lo, hi, ok):
    """The largest x in [lo, hi) with ok(x), for ok true at lo and false at hi."""
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def _plan(shape, policy=A, mode=REF, has_init=0):
    return {"fn": "plan", "shape": list(shape), "policy": policy, "mode": mode, "has_init": has_init}


def queries(L):
    """The questions.  The four shapes either side of a byte bound are found by
    asking `L` itself (bisection on the literal or clause count)."""
    def fits_lds(l):
        return L.satmi_dpll_lds_bytes(2000, 6000, l) > 0

    def fits_scan(c):
        return L.satmi_dpll_scan_lds_bytes(600, c, 3 * c, 5) > 0

    def fits_4g(l):
        return ask(L, _plan((10, 10, l, 3), W))["rc"] == _capi.OK

    l160 = _last_true(0, 65535, fits_lds)           # the last literal count under 160 KiB at 2000 x 6000
    c160 = _last_true(1, 21000, fits_scan)          # the last clause count of the clause kernels' image
    l4g = _last_true(10, 1 << 30, fits_4g)          # the last literal count under 4 GiB per wave
    narrow = [(0, 0, 0), (1, 1, 1), (50, 213, 639), (32766, 10, 10), (32767, 10, 10), (10, 65534, 10),
              (10, 65535, 10), (10, 10, 65535), (10, 10, 65536), (2000, 6000, l160), (2000, 6000, l160 + 1),
              (-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    rng = random.Random(20)
    narrow += [(rng.randint(0, 4000), rng.randint(0, 12000), rng.randint(0, 50000)) for _ in range(6)]
    out = [{"fn": "lds_bytes", "shape": list(s) + [0]} for s in narrow]
    # either side of everything the general kernel's choice turns on, under the
    # (policy, mode, has_init) that keep the clause kernels out (the first four
    # of them past the first four shapes)
    edges = [(20, 60, 180, 3), (20, 60, 180, 0), (300, 40, 12000, 255), (300, 40, 12000, 256),
             (32766, 10, 10, 3), (32767, 10, 10, 3), (10, 65534, 10, 3), (10, 65535, 10, 3),
             (10, 10, 65535, 3), (10, 10, 65536, 3), (2000, 6000, l160, 3), (2000, 6000, l160 + 1, 3)]
    for i, shape in enumerate(edges):
        out += [_plan(shape, *pmh) for pmh in NO_CLAUSE_KERNEL[:8 if i < 4 else 4]]
    # the LDS shape classes (4, 2, 1 waves per workgroup) of the narrow form
    out += [_plan(s) for s in ((100, 426, 1278, 3), (1500, 4500, 13500, 3), (2500, 9000, 27000, 3))]
    # the wide form's limits, and either side of 4 GiB per wave
    big = [((1 << 30) - 2, 10, 10, 3), ((1 << 30) - 1, 10, 10, 3), (10, 1 << 28, 10, 3), (10, (1 << 28) + 1, 10, 3),
           (10, 10, 1 << 30, 3), (10, 10, (1 << 30) + 1, 3), (10, 10, l4g, 3), (10, 10, l4g + 1, 3),
           (1 << 26, 1 << 24, 1 << 26, 3), (1 << 27, 1 << 25, 1 << 27, 300)]
    for shape in big:
        out += [_plan(shape, A), _plan(shape, G, SOUND, 0)]
    # the clause kernels' eligibility: clause lengths 0..6, the variable limits
    # of the two packings, the literal and clause limits, the image's byte bound
    scan = [(50, 213, 639, k) for k in range(7)]
    scan += [(511, 100, 300, 3), (512, 100, 300, 3), (2047, 100, 500, 5), (2048, 100, 500, 5), (2047, 100, 300, 3),
             (100, 65534, 65535, 3), (100, 65535, 65535, 3), (100, 100, 65535, 5), (100, 100, 65536, 5),
             (600, c160, 3 * c160, 5), (600, c160 + 1, 3 * (c160 + 1), 5), (100, 8191, 24573, 3),
             (100, 8192, 24576, 3), (-1, 10, 10, 3), (10, -1, 10, 3)]
    out += [{"fn": "scan_lds_bytes", "shape": list(s)} for s in scan]
    return out
