"""Resolution saturation (csrc/resolution.hip) through its regrowth and layout
paths: the packed path's stage spill, key-room overflow and RES_ABUF overflow
on a fresh workspace, unrecorded batches, clause_limit and the record's
truncation on both paths, every key width of the general path's pair kernel,
its mid-j buffer flush, and a pass of two chunks with a mid-pass table
rebuild -- each counted by satmi_resolution_last_regrowths.

The rows and what each reaches are in tests/res_paths.py, proven on the CPU
by tests/test_res_paths.py.  Every comparison is exact: against the plain
construction {S_i u T_j} for the product rows (the oracle needs seconds for
them and agrees, on the CPU side), against the oracle elsewhere, against
tests/golden/resolution_php43.json for the three copies of PHP(4,3).  An
unrecorded call returns no clauses: it is compared in all it returns (the
verdict, the passes, every pass's count), and a recorded call closes each
sequence on the same workspace.  No time limits."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import oracle
import res_paths as P
from conftest import clause_set_sha
from satmi import _capi
from satmi.resolution import _csr, _p, last_stats, resolve

pytestmark = pytest.mark.gpu

ZERO = dict.fromkeys(_capi.RES_REGROWTHS, 0)


def regrowths():
    return last_stats()["regrowths"]


def packed(**kw):
    return dict(ZERO, **kw)


# what a fresh workspace must regrow in the row's first call (res_paths.model)
PACKED_FIRST = {"stage_one_stripe": packed(stage=1), "stage_present": packed(stage=1), "keys_even": packed(keys=1), "abuf": packed(stage=1)}


@pytest.mark.parametrize("name", list(P.PRODUCT_ROWS))
def test_packed_regrowth_rows(name):
    """A fresh workspace regrows once, for the reason the model gives, and the
    pass run again adds exactly the construction (a table re-seeded wrongly
    would find every key present and answer True with no pass; one not
    re-seeded would add stage_present's 20 resolvents that are input clauses).  On the
    regrown workspace nothing regrows: unrecorded (a batch of 4), once more
    (the batch launched from its captured graph), recorded again -- abuf's
    direct appends now stored by the first run of the pass.  Then fresh again
    and unrecorded: the regrowth inside a batch."""
    f, want = P.row(name)
    _capi.trim_workspaces()
    t = time.perf_counter()
    r = resolve(f, record=True)
    first = regrowths()
    assert (r["result"], r["passes"], r["pass_new"]) == (1, 1, [len(want)]), name
    assert r["clauses"] == [want], name
    assert first == PACKED_FIRST[name], (name, first)
    for k in range(2):
        u = resolve(f)
        assert (u["result"], u["passes"], u["pass_new"]) == (1, 1, [len(want)]), (name, k)
        assert regrowths() == ZERO, (name, k)
    r = resolve(f, record=True)
    assert (r["result"], r["pass_new"]) == (1, [len(want)]) and r["clauses"] == [want], name
    assert regrowths() == ZERO, name
    _capi.trim_workspaces()
    u = resolve(f)
    again = regrowths()
    assert (u["result"], u["passes"], u["pass_new"]) == (1, 1, [len(want)]), name
    assert again == first, (name, again)
    r = resolve(f, record=True)
    assert r["clauses"] == [want] and regrowths() == ZERO, name
    print(name, "fresh", first, "second call", ZERO, "%.2f s" % (time.perf_counter() - t))


def same(r, o):
    return (r["result"], r["passes"], r["pass_new"]) == (o["result"], o["passes"], o["pass_new"])


def test_unrecorded_batches_chain30():
    """Five adding passes and the empty sixth, unrecorded: a first batch of 4
    (enqueued, then captured, then replayed), a second launched plainly, the
    verdict in its middle.  max_passes = 20: one batch of 16; 3, 5: the bound
    ends the batch (result -1); 6: the empty pass is the last allowed."""
    f = P.chain(30)
    o = oracle.resolution(f, record=True)
    assert o["pass_new"] == [29, 55, 98, 148, 105]
    _capi.trim_workspaces()
    for k in range(4):
        assert same(resolve(f), o), k
        assert regrowths() == ZERO
    for mp in (20, 3, 5, 6):
        om = oracle.resolution(f, max_passes=mp)
        assert om["result"] == (1 if mp > 5 else -1)
        for k in range(3):
            assert same(resolve(f, max_passes=mp), om), (mp, k)
    r = resolve(f, record=True)
    assert same(r, o) and r["clauses"] == [sorted(p) for p in o["clauses"]]
    assert same(resolve(f), o)


@pytest.mark.parametrize("n", [30, 40])
def test_clause_limit(n):
    """clause_limit on the packed (30 variables) and the general path (40):
    the saturation stops after the first pass p that brings the clause count
    over the limit -- passes and counts are the oracle's with max_passes = p
    (the oracle's own clause_limit stops in the middle of that pass, so it is
    not the comparison); a limit the saturation never exceeds changes nothing.
    Unrecorded three times (batches), then recorded."""
    f = P.chain(n)
    full = oracle.resolution(f, record=True)
    for lim, p in P.limit_cases(full["pass_new"], n):
        o = full if p is None else oracle.resolution(f, max_passes=p, record=True)
        if p is not None:
            assert o["result"] == -1 and o["passes"] == p
        for k in range(3):
            assert same(resolve(f, clause_limit=lim), o), (n, lim, k)
        r = resolve(f, clause_limit=lim, record=True)
        assert same(r, o) and r["clauses"] == [sorted(c) for c in o["clauses"]], (n, lim)
        assert same(resolve(f, clause_limit=lim, max_passes=20), o), (n, lim)


GUARD = -7777777


def raw_resolve(f, lit_cap, clause_cap, rec_pass_cap, pass_cap=64, pad=64):
    """satmi_resolution_host with record arrays of exactly these capacities,
    each followed by `pad` guard words.  Returns (result, passes, pass_new,
    recorded passes) after asserting every guard word is untouched."""
    L = _capi.load()
    off, lits = _csr(f)
    res, passes = ctypes.c_int32(0), ctypes.c_int32(0)
    pn = np.full(pass_cap + pad, GUARD, dtype=np.int64)
    rl = np.full(lit_cap + pad, GUARD, dtype=np.int32)
    rco = np.full(clause_cap + pad, GUARD, dtype=np.int64)
    rpo = np.full(rec_pass_cap + pad, GUARD, dtype=np.int64)
    _capi.check(L.satmi_resolution_host(len(f), _p(off), _p(lits), 0, 0, 0.0, ctypes.byref(res), ctypes.byref(passes),
                                        _p(pn, ctypes.c_int64), pass_cap, _p(rl), lit_cap, _p(rco, ctypes.c_int64),
                                        clause_cap, _p(rpo, ctypes.c_int64), rec_pass_cap), "satmi_resolution_host")
    for a, cap in ((pn, pass_cap), (rl, lit_cap), (rco, clause_cap), (rpo, rec_pass_cap)):
        assert (a[cap:] == GUARD).all(), "written past an array's capacity"
    rec = []
    for p in range(min(passes.value, rec_pass_cap - 1)):
        rec.append([rl[rco[c]:rco[c + 1]].tolist() for c in range(rpo[p], rpo[p + 1])])
    return res.value, passes.value, pn[:passes.value].tolist(), rec


def truncated(want, lit_cap, clause_cap, rec_pass_cap):
    """include/satmi.h's rule on the oracle's sorted passes: a pass's record
    stops before the first clause that does not fit."""
    out, ncl, nl = [], 0, 0
    for p in want[:max(rec_pass_cap - 1, 0)]:
        got = []
        for c in p:
            if ncl + 1 >= clause_cap or nl + len(c) > lit_cap:
                break
            got.append(c)
            ncl, nl = ncl + 1, nl + len(c)
        out.append(got)
    return out


@pytest.mark.parametrize("n", [30, 40])
def test_record_truncation(n):
    """Record arrays too small for pass 3 (by literals, by clauses), or with
    room for two passes only: the verdict, the passes and every pass_new are
    those of the full run, each recorded pass is a prefix of the oracle's
    sorted pass (passes 1-2 whole, pass 3 cut), and no word after an array's
    capacity is written.  Packed (30 variables) and general (40)."""
    f = P.chain(n)
    o = oracle.resolution(f, record=True)
    want = [sorted(p) for p in o["clauses"]]
    size = [sum(map(len, p)) for p in want]
    full = raw_resolve(f, 1 << 16, 1 << 16, 64)
    assert full == (o["result"], o["passes"], o["pass_new"], want)
    cases = ((size[0] + size[1] + size[2] // 2, 1 << 16, 64),                       # literals run out in pass 3
             (1 << 16, len(want[0]) + len(want[1]) + len(want[2]) // 2, 64),        # clause offsets run out in pass 3
             (1 << 16, 1 << 16, 3),                                                 # passes 1-2 only
             (1 << 16, 1 << 16, 1), (1, 1, 64))
    for lit_cap, clause_cap, rec_pass_cap in cases:
        for k in range(2):
            res, passes, pn, rec = raw_resolve(f, lit_cap, clause_cap, rec_pass_cap)
            assert (res, passes, pn) == (o["result"], o["passes"], o["pass_new"]), (n, lit_cap, clause_cap)
            for p, got in enumerate(rec):
                assert got == want[p][:len(got)], (n, p)
            assert rec == truncated(want, lit_cap, clause_cap, rec_pass_cap), (n, lit_cap, clause_cap, rec_pass_cap)
    res, passes, pn, rec = raw_resolve(f, *cases[0])
    assert rec[:2] == want[:2] and 0 < len(rec[2]) < len(want[2])
    res, passes, pn, rec = raw_resolve(f, *cases[1])
    assert rec[:2] == want[:2] and 0 < len(rec[2]) < len(want[2])


@pytest.mark.parametrize("V", P.WIDTHS)
def test_key_widths(V):
    """W = 1, 2, 2, 3, 3, 4, 4 (their own instances of res_pairs_kernel) and
    5, 5, 16 (the run-time width), with resolvents on the variables at bit 63
    of a word, bit 0 of the next, and in the last word: three passes,
    recorded, every pass's set against the oracle; then unrecorded."""
    f, _ = P.row("width_%d" % V)
    o = oracle.resolution(f, max_passes=3, record=True)
    r = resolve(f, max_passes=3, record=True)
    assert same(r, o), V
    assert r["clauses"] == [sorted(p) for p in o["clauses"]], V
    g = regrowths()
    assert (g["stage"], g["keys"], g["table"], g["chunks"], g["cand_reruns"]) == (0, 0, 0, 3, 0), g
    assert same(resolve(f, max_passes=3), o), V


@pytest.mark.parametrize("name", list(P.PAIRBUF_ROWS))
def test_pair_buffer_flush_inside_a_clause(name):
    """The last clause has 2,600 candidates: its workgroup flushes a full
    PAIR_BUF (2,048) in the middle of its walk and the rest at the end, at
    W = 2 and at the run-time width.  Exactly the 2,600 clauses [y_a, y_b]."""
    f, want = P.row(name)
    for record in (True, False, True):
        r = resolve(f, record=record)
        assert (r["result"], r["passes"], r["pass_new"]) == (1, 1, [2600]), name
        if record:
            assert r["clauses"] == [want], name
        assert last_stats()["candidates"] == 2600
        assert regrowths()["chunks"] == 2 and regrowths()["cand_reruns"] == 0


def test_php43x3_two_chunks_and_a_table_rebuild(golden_dir):
    """Three disjoint copies of PHP(4,3) (36 variables: the general path),
    four passes, recorded.  Pass 4 runs over 22,380 clauses -- 2.5e8 pairs, two
    chunks, the second's winners appended behind the first's -- and adds
    3 x 163,954 clauses through a table rebuilt in the middle of the pass and
    a clause buffer that grows in every pass.  No clause mixes copies; each
    copy's clauses, renamed to copy 0, are the reference's own for the single
    formula: passes 1-3 clause by clause, pass 4 by the sha256 of the set.
    The second call grows nothing."""
    with open(os.path.join(golden_dir, "resolution_php43.json")) as fh:
        (c,) = json.load(fh)["cases"]
    f, _ = P.row("php43x3")
    counts = [3 * p["count"] for p in c["passes"]]
    assert counts == [108, 810, 21396, 491862]
    _capi.trim_workspaces()
    t = time.perf_counter()
    r = resolve(f, max_passes=4, record=True, rec_cap=1 << 24)
    dt = time.perf_counter() - t
    first = regrowths()
    print("php43x3 recorded call %.2f s" % dt, first)
    assert (r["result"], r["passes"], r["pass_new"]) == (-1, 4, counts)
    for k, p in enumerate(c["passes"]):
        assert len(r["clauses"][k]) == counts[k], k
        for part in P.php_project(r["clauses"][k]):      # raises on a clause that mixes copies
            assert len(part) == p["count"], k
            if "clauses" in p:
                assert sorted(part) == p["clauses"], k
            assert clause_set_sha(part) == p["sha256"], k
    assert (first["stage"], first["keys"], first["table"], first["cand_reruns"]) == (0, 0, 0, 0), first
    assert first["chunks"] == 3 + 2, first               # passes 1-3 one chunk each, pass 4 two
    assert first["table_rebuilds"] >= 1 and first["clause_growths"] >= 4, first
    u = resolve(f, max_passes=4)
    second = regrowths()
    print("php43x3 second call", second)
    assert (u["result"], u["passes"], u["pass_new"]) == (-1, 4, counts)
    assert second == dict(first, clause_growths=0), second
