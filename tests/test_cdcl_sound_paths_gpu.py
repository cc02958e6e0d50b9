"""GPU checks of the sound CDCL's four kernels (csrc/cdcl_sound_search.inc) at the path rows of
tests/cdcl_sound_paths.py, whose witnesses tests/test_cdcl_sound_paths.py asserts on the CPU:
past 256 conflicts, past lane 63 with activities and gaps in the ids, past 64 unmarked trail
entries in each of the three walks, past level 255.  The kernel is the Python rule word for
word -- status, the eight counters, model row, core, lemma list, record counts, and for the
carrying and shrinking entry points the kept lemmas and the chain's words -- through
cdcl_sound_batch, cdcl_assume_batch, cdcl_carry_batch and cdcl_shrink_batch, in both clause
forms and with one wave taking the rows in turn; and every answer passes the library's own
checkers."""
import functools

import pytest

import cdcl_carry_rows as C
import cdcl_shrink_rows as S
import cdcl_sound_paths as P
import cdcl_sound_rows as R
from satmi import cdcl_sound
from satmi.check import check_models
from satmi.refute import check_refutations, proof_of_cdcl, proof_of_cdcl_assumed, trim_refutations
from test_cdcl_assume_gpu import _same as _assume_same
from test_cdcl_carry_gpu import _host_same as _carry_same
from test_cdcl_shrink_gpu import _host_same as _shrink_same
from test_cdcl_sound_gpu import _same as _sound_same

pytestmark = pytest.mark.gpu

ROW = {r[0]: r for r in P.rows()}
NAMES = list(ROW)
FIRST_SLICE = "resumed: the first slice"        # the one row with a conflict_limit: a launch of its own
FREE = [n for n in NAMES if not ROW[n][4]]
PLAIN = [n for n in FREE if not ROW[n][2] and not ROW[n][3]]       # no assumptions, nothing carried
UNCARRIED = [n for n in FREE if not ROW[n][3]]
ASSUMING = [n for n in FREE if ROW[n][2]]


def _short(names):
    return [n for n in names if max(map(len, ROW[n][1])) <= R.SHORT_MAX]


# "all" holds `level 300` and a 12-literal clause: the wave-per-clause form; "short" is the
# lane-per-clause form; grid 1 = one wave takes the rows in turn, so `act`, `seen` and `flags`
# beyond 64 variables are cleared between instances that used them
FORMS = [("all", 0), ("short", 0), ("short", 1)]
ROOM = (8192, 131072)       # proof and kept arrays that hold every row: no call runs twice


def _group(names, form):
    return list(names) if form == "all" else _short(names)


def _units(lits):
    return [[l] for l in lits]


def _chain_want(name):
    """The shrinking rule's result: without assumptions query 0 cannot end ASSUMED, and the result
    is the carrying rule's with one query counted (test_cdcl_sound_paths.py holds the two equal)."""
    return P.want(name, "shrink") if ROW[name][2] else dict(P.want(name), shrink=[1, 0, 0, 0, 0, 0])


def _call(entry, names, grid, assumed=True, limit=0):
    f = [ROW[n][1] for n in names]
    a = [ROW[n][2] if assumed else [] for n in names]
    carry = [ROW[n][3] for n in names]
    cdcl_sound.debug_grid(grid, 1 if grid else 0)
    try:
        if entry == "sound":
            res = cdcl_sound.cdcl_sound_batch(f, conflict_limit=limit, room=ROOM)
        elif entry == "assume":
            res = cdcl_sound.cdcl_assume_batch(f, a, conflict_limit=limit, room=ROOM)
        elif entry == "carry":
            res = cdcl_sound.cdcl_carry_batch(f, a, carry, conflict_limit=limit, room=ROOM)
        else:
            res = cdcl_sound.cdcl_shrink_batch(f, a, carry, conflict_limit=limit, room=ROOM)
    finally:
        cdcl_sound.debug_grid(0, 0)
    return dict(zip(names, res))


@functools.lru_cache(maxsize=None)
def got(entry, form, grid, assumed=True):
    """One host call on the entry point's rows: name -> its dict."""
    names = {"sound": PLAIN, "assume": UNCARRIED if assumed else ASSUMING,
             "carry": FREE if assumed else ASSUMING, "shrink": FREE}[entry]
    return _call(entry, _group(names, form), grid, assumed)


def test_the_groups_hold_what_they_are_for():
    for names in (PLAIN, UNCARRIED, FREE):
        assert max(max(map(len, ROW[n][1])) for n in names) > R.SHORT_MAX
        for n in ("php 6", "two halvings", "uip gap", "low gap", "opposite offers in one step",
                  "opposite offers 64 clauses apart") + tuple(f"renamed {i}" for i in P.RENAMED):
            assert n in _short(names), n
        assert "level 300" not in _short(names) and "opposite offers beside a long clause" not in _short(names)
    assert set(P.CHAIN_ROWS) | {"final gap"} == set(ASSUMING) and ASSUMING == _short(ASSUMING)
    assert "resumed" in _short(FREE) and "resumed" not in UNCARRIED and FIRST_SLICE not in FREE


@pytest.mark.parametrize("form,grid", FORMS)
def test_sound_kernel_is_the_python_rule(form, grid):
    res = got("sound", form, grid)
    for n in _group(PLAIN, form):
        _sound_same(n, res[n], P.want(n))


@pytest.mark.parametrize("form,grid", FORMS)
def test_assume_kernel_is_the_python_rule(form, grid):
    res = got("assume", form, grid)
    for n in _group(UNCARRIED, form):
        _assume_same(n, res[n], P.want(n))


@pytest.mark.parametrize("form,grid", FORMS)
def test_carry_kernel_is_the_python_rule(form, grid):
    """(Here the lemma list of a SAT row is compared too: it is the kept list.)"""
    res = got("carry", form, grid)
    for n in _group(FREE, form):
        _carry_same(n, res[n], P.want(n))
        _assume_same(n, res[n], P.want(n))      # (and the core's length, the record count by the lemma list)


@pytest.mark.parametrize("form,grid", FORMS)
def test_shrink_kernel_is_the_python_rule(form, grid):
    """The chain rows, and every other row, where the shrinking kernel is the carrying one with
    the chain's words [1, 0, 0, 0, 0, 0]."""
    res = got("shrink", form, grid)
    for n in _group(FREE, form):
        _shrink_same(n, res[n], _chain_want(n))
    for n in P.CHAIN_ROWS:
        assert res[n]["shrink"]["queries"] >= 8 and res[n]["counters"]["conflicts"] == 284


@pytest.mark.parametrize("entry", ["assume", "carry"])
def test_rows_with_assumptions_also_run_without_them(entry):
    res = got(entry, "short", 0, False)
    for n in ASSUMING:
        w = P.want(n, "carry", False)
        assert w["status"] == C.SAT, n       # (the selectors and the assumed literals are free: every one is satisfiable)
        (_assume_same if entry == "assume" else _carry_same)(n, res[n], w)


def test_the_first_slice_ends_limit_in_all_four():
    """`resumed` carries what this query keeps: LIMIT at 200 conflicts, 199 lemmas."""
    w = P.want(FIRST_SLICE)
    assert w["status"] == C.LIMIT and w["counters"][0] == P.RESUME_AT and len(w["kept"]) == P.RESUME_AT - 1
    for entry in ("sound", "assume", "carry", "shrink"):
        g = _call(entry, [FIRST_SLICE, "uip gap"], 0, limit=P.RESUME_AT)
        _sound_same(FIRST_SLICE, g[FIRST_SLICE], w)
        _sound_same("uip gap", g["uip gap"], P.want("uip gap"))
        if entry in ("carry", "shrink"):
            assert g[FIRST_SLICE]["kept"] == w["kept"] == ROW["resumed"][3]


def test_the_shrinking_kernel_is_the_host_side_chain_over_the_carrying_entry_point():
    def query(f, a, limit, carry):
        return cdcl_sound.cdcl_carry_batch([f], [a], [carry], conflict_limit=limit, room=ROOM)[0]
    res = got("shrink", "short", 0)
    for n in P.CHAIN_ROWS:
        _, f, a, carry, limit = ROW[n]
        status, core, kept, total = S.host_chain(query, f, a, limit, carry)
        g = res[n]
        assert (g["status"], g["core"], g["kept"]) == (status, core, kept), n
        assert [g["counters"][k] for k in S.COUNTERS] == total, n


@pytest.mark.parametrize("entry", ["sound", "assume", "carry", "shrink"])
def test_every_answer_is_certified_by_the_librarys_checkers(entry):
    res = got(entry, "all", 0)
    names = list(res)
    sat = [n for n in names if res[n]["sat"]]
    refuted = [n for n in names if res[n]["sat"] is False]
    assert len(sat) + len(refuted) == len(names) and len(sat) >= 8 and len(refuted) >= 6
    models = check_models([ROW[n][1] + _units(ROW[n][2]) for n in sat], [[res[n]["model"]] for n in sat])
    for n, c in zip(sat, models):
        assert c[0]["ok"], n
    if entry == "sound":
        fs, ps = [ROW[n][1] for n in refuted], [proof_of_cdcl(res[n]) for n in refuted]
    else:       # (a carried lemma stands in the proof, in front: the check holds it to the formula too)
        pairs = [proof_of_cdcl_assumed(ROW[n][1], res[n]) for n in refuted]
        fs, ps = [p[0] for p in pairs], [p[1] for p in pairs]
    for n, c, t in zip(refuted, check_refutations(fs, ps), trim_refutations(fs, ps)):
        assert c["proven"] and c["failed"] == 0, n
        assert t["proven"], n
