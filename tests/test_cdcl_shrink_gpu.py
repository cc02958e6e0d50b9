"""GPU checks of minimal failed-assumption cores (csrc/cdcl_sound.hip's shrinking kernel and its
host form) at the rows of tests/cdcl_shrink_rows.py: the kernel is the Python rule exactly --
status, counters, info, shrink_info, core, model row, the region's words and carry_out -- in
both clause forms, on the default grid and with one wave taking every instance in turn, with
core_stride 0 and with the full stride; it is the same chain run from the host over
satmi_cdcl_carry_batch_host; where query 0 does not end ASSUMED it is the carrying entry point
word for word; and its answers pass the library's own checkers."""
import functools

import numpy as np
import pytest

import cdcl_carry_rows as C
import cdcl_shrink_rows as S
import cdcl_sound_rows as R
from satmi import _capi, cdcl_sound, check, incremental, refute, solvers
from satmi.cnf import pack

pytestmark = pytest.mark.gpu

GUARD, NG = 0x5A5A5A5A, 8
ROWS = S.rows()
ROW = {r[0]: r for r in ROWS}
NAMES = [r[0] for r in ROWS]
SHORT = [n for n in NAMES if max([len(c) for c in ROW[n][1]] + [0]) <= R.SHORT_MAX]
CSTRIDE = max(len(r[2]) for r in ROWS)
WORDS = ("status", "counters", "row_len", "row_lits", "core_len", "core_lits", "info", "carry", "lemmas")


def _units(lits):
    return [[l] for l in lits]


def spec(name, limit=None):
    """One instance of a launch: its region is exactly what the chain needs (or the row's room),
    the carried records at its head.  `limit` = the launch's conflict_limit where it is not the
    row's own."""
    _, f, a, carry, room, nv = ROW[name]
    w = S.want(ROW[name]) if limit is None else S.solve(f, a, limit, carry, room, nv)
    if room is None:
        room = max(w["words"], w["first"]["words"], R.region_words(carry))
    if nv is None:
        nv = max([abs(l) for c in list(f) + list(carry) for l in c] + [abs(l) for l in a] + [0])
    return dict(f=f, a=a, carry=carry, room=room, nv=nv, want=w)


class Launch:
    """satmi_cdcl_shrink_batch_device (or, with entry="carry", satmi_cdcl_carry_batch_device) on
    torch tensors.  Every region is exactly its room, guard words behind what lies there and
    behind the last region, the core rows and the scratch."""

    def __init__(self, specs, limit=0, grid=0, short=False, core_stride=CSTRIDE, entry="shrink"):
        import torch
        self.specs, self.B = specs, len(specs)
        B, dev = self.B, torch.device("cuda", 0)
        batch = pack([s["f"] for s in specs])
        begin, alits, _ = cdcl_sound.pack_assumptions([s["a"] for s in specs], B)
        nv = max([s["nv"] for s in specs] + [0])
        mlen = max([len(c) for s in specs for c in s["f"]] + [0])
        assert not short or 1 <= mlen <= R.SHORT_MAX
        self.lb = lb = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([s["room"] for s in specs], out=lb[1:])
        region = np.full(int(lb[-1]) + NG, GUARD, dtype=np.int64)
        for b, s in enumerate(specs):
            rec = C.records(s["carry"])
            region[lb[b]:lb[b] + len(rec)] = rec
        self.before = region.astype(np.int32)
        self.stride, self.cstride, self.natot = max(nv, 1), core_stride, int(begin[-1])
        cin = np.array([(len(s["carry"]), R.region_words(s["carry"])) for s in specs], dtype=np.int64).reshape(-1)

        def up(a, dt=np.int32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

        def filled(n, dt=torch.int32):
            return torch.full((n,), GUARD, dtype=dt, device=dev)

        t = [up(batch.inst_clause_begin), up(batch.clause_lit_begin), up(batch.lits), up([s["nv"] for s in specs])]
        d_lb, d_ab, d_al = up(lb, np.int64), up(begin), up(alits)
        self.lemmas = up(self.before)
        self.status, self.counters = filled(B), filled(B * 8, torch.int64)
        self.row_len, self.row_lits = filled(B), torch.zeros(B * self.stride, dtype=torch.int32, device=dev)
        self.core_len, self.core_lits = filled(B), filled(B * core_stride + NG)
        self.info = filled(B * 4, torch.int64)
        self.carry = torch.cat([up(cin, np.int64), filled(NG, torch.int64)])
        self.work = filled(2 * self.natot + NG)
        self.shrink = filled(B * 6 + NG, torch.int64)
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (B, *(x.data_ptr() for x in t), nv, mlen, self.lemmas.data_ptr(), d_lb.data_ptr(),
                self.status.data_ptr(), self.counters.data_ptr(), self.row_len.data_ptr(), self.row_lits.data_ptr(),
                self.stride, self.info.data_ptr(), d_ab.data_ptr(), d_al.data_ptr(), self.core_len.data_ptr(),
                self.core_lits.data_ptr() if core_stride else None, core_stride, self.carry.data_ptr(),
                self.carry.data_ptr())
        cdcl_sound.debug_grid(grid, 1 if grid else 0)
        try:
            if entry == "carry":
                cdcl_sound.cdcl_carry_device(*args, conflict_limit=limit, stream=stream)
            else:
                cdcl_sound.cdcl_shrink_device(*args, self.work.data_ptr(), self.shrink.data_ptr(),
                                              conflict_limit=limit, stream=stream)
        finally:
            cdcl_sound.debug_grid(0, 0)
        torch.cuda.current_stream(dev).synchronize()
        o = {k: getattr(self, k).cpu().numpy() for k in WORDS + ("work", "shrink")}
        assert (o["core_lits"][B * core_stride:] == GUARD).all() and (o["carry"][2 * B:] == GUARD).all()
        assert (o["lemmas"][lb[-1]:] == GUARD).all() and (o["work"][2 * self.natot:] == GUARD).all()
        assert (o["shrink"][6 * B:] == GUARD).all()
        o["counters"], o["info"], o["carry"] = o["counters"].reshape(B, 8), o["info"].reshape(B, 4), o["carry"][:2 * B].reshape(B, 2)
        o["row_lits"] = o["row_lits"].reshape(B, self.stride)
        o["core_lits"] = o["core_lits"][:B * core_stride].reshape(B, core_stride)
        o["shrink"] = o["shrink"][:6 * B].reshape(B, 6)
        self.o = o

    def region(self, b, o=None):
        return (o or self.o)["lemmas"][self.lb[b]:self.lb[b + 1]].tolist()


def _same(name, L, b, w):
    """Instance b of a launch against the rule's result `w`."""
    o = L.o
    assert o["status"][b] == w["status"], name
    assert o["counters"][b].tolist() == w["counters"], name
    assert o["shrink"][b].tolist() == w["shrink"], name
    assert o["info"][b, :3].tolist() == [w["records"], w["words"], w["flags"]], name
    model = w["model"] or []
    assert o["row_len"][b] == len(model) and o["row_lits"][b, :len(model)].tolist() == model, name
    core = (w["core"] or []) if w["status"] == S.ASSUMED else []
    k = min(len(core), L.cstride)
    assert o["core_len"][b] == len(core) and o["core_lits"][b, :k].tolist() == core[:k], name
    if w["status"] == S.ASSUMED:       # 0 behind the core as far as query 0's reached, and nothing further
        first = min(w["shrink"][4], L.cstride)
        assert not o["core_lits"][b, k:first].any() and (o["core_lits"][b, first:] == GUARD).all(), name
    before = L.before[L.lb[b]:L.lb[b + 1]].tolist()
    if w["status"] == S.TOO_LARGE:
        assert L.region(b) == before and o["carry"][b].tolist() == [len(L.specs[b]["carry"]), R.region_words(L.specs[b]["carry"])], name
        return
    rec = C.records(w["lemmas"])
    got = L.region(b)
    assert got[:len(rec)] == rec, name
    # behind the records: untouched, or the closing record of an earlier query (one word)
    assert all(x == y or x == 0 for x, y in zip(got[len(rec):], before[len(rec):])), name
    assert o["carry"][b].tolist() == [len(w["kept"]), R.region_words(w["kept"])], name


@functools.lru_cache(maxsize=None)
def launch(group, grid, core_stride, limit=0):
    names = [n for n in (NAMES if group == "all" else SHORT) if S.LIMITS.get(n, 0) == limit]
    specs = [spec(n) for n in names]
    if limit:      # (neighbours, so the one-wave grid has other instances in front and behind)
        names = ["hand row"] + names + ["unsat trial"]
        specs = [spec(names[0], limit)] + specs + [spec(names[-1], limit)]
    return names, Launch(specs, limit=limit, grid=grid, short=group == "short", core_stride=core_stride)


@pytest.mark.parametrize("group,grid,core_stride", [("all", 0, CSTRIDE), ("short", 0, CSTRIDE), ("short", 1, CSTRIDE),
                                                    ("all", 1, 0), ("short", 0, 0), ("short", 0, 2)])
def test_kernel_is_the_python_rule(group, grid, core_stride):
    """Every row, in the wave-per-clause form ("all": a 69-literal clause is among them) and the
    lane-per-clause form ("short"), on the default grid and with one wave taking every formula in
    turn (grid 1 x 1): the clean-up between queries and between instances; with no core row
    (core_stride 0), a short one and the full one."""
    assert len(SHORT) == len(NAMES) - 1 and CSTRIDE == 70
    for limit in sorted(set(S.LIMITS.values()) | {0}):
        names, L = launch(group, grid, core_stride, limit)
        for b, n in enumerate(names):
            _same(n, L, b, L.specs[b]["want"])
    L = launch(group, grid, core_stride)[1]
    assert {s["want"]["status"] for s in L.specs} == {S.UNSAT, S.SAT, S.FULL, S.TOO_LARGE, S.ASSUMED}
    assert any(s["want"]["shrink"][3] for s in launch(group, grid, core_stride, max(S.LIMITS.values()))[1].specs)


def test_outputs_do_not_depend_on_the_grid_the_form_or_the_core_stride():
    (names, a), (_, b) = launch("short", 0, CSTRIDE), launch("short", 1, CSTRIDE)
    _, c = launch("short", 0, 0)
    _, d = launch("all", 0, CSTRIDE)
    for k in WORDS + ("shrink",):
        assert np.array_equal(a.o[k], b.o[k]), k
        if k != "core_lits":
            assert np.array_equal(a.o[k], c.o[k]), k
    at = {n: i for i, n in enumerate(launch("all", 0, CSTRIDE)[0])}
    for i, n in enumerate(names):
        for k in ("status", "counters", "core_len", "core_lits", "info", "carry", "shrink", "row_len"):
            assert np.array_equal(a.o[k][i], d.o[k][at[n]]), (n, k)
        assert a.region(i) == d.region(at[n]), n


def test_where_query_0_is_not_assumed_every_output_is_the_carrying_entry_points():
    """With no assumptions anywhere (the rows' formulas as they are), and at every row whose
    query 0 ends otherwise: word for word satmi_cdcl_carry_batch_device's."""
    bare = [dict(spec(n), a=[]) for n in NAMES if ROW[n][4] is None]
    for s in bare:
        s["room"] = max(C.solve(s["f"], [], 0, s["carry"], None, s["nv"])["words"], R.region_words(s["carry"]))
    old, new = Launch(bare, entry="carry"), Launch(bare)
    for k in WORDS:
        assert np.array_equal(old.o[k], new.o[k]), k
    assert new.o["shrink"].tolist() == [[1, 0, 0, 0, 0, 0]] * len(bare)
    assert {S.SAT, S.UNSAT} <= set(new.o["status"].tolist()) and any(s["carry"] for s in bare)
    names, new = launch("all", 0, CSTRIDE)
    old = Launch(new.specs, entry="carry")
    rest = [b for b, s in enumerate(new.specs) if s["want"]["first"]["status"] != S.ASSUMED]
    assert {new.specs[b]["want"]["status"] for b in rest} == {S.SAT, S.UNSAT, S.TOO_LARGE}
    for b in rest:
        for k in ("status", "counters", "row_len", "row_lits", "core_len", "core_lits", "info", "carry"):
            assert np.array_equal(old.o[k][b], new.o[k][b]), (names[b], k)
        assert old.region(b) == new.region(b), names[b]


# ---- the host form
HOST = [n for n in NAMES if ROW[n][4] is None and ROW[n][5] is None and n not in S.LIMITS]


@functools.lru_cache(maxsize=None)
def host_results():
    return cdcl_sound.cdcl_shrink_batch([ROW[n][1] for n in HOST], [ROW[n][2] for n in HOST], [ROW[n][3] for n in HOST])


def _host_same(name, g, w):
    assert g["status"] == w["status"], name
    assert [g["counters"][k] for k in S.COUNTERS] == w["counters"], name
    assert g["model"] == w["model"] and g["kept"] == w["kept"], name
    assert (g["records"], g["region_words"], g["flags"]) == (w["records"], w["words"], w["flags"]), name
    assert [g["shrink"][k] for k in S.SHRINK] == w["shrink"], name
    if w["status"] in (S.UNSAT, S.ASSUMED):
        assert g["proof"] == w["lemmas"] and g["core"] == w["core"] and g["core_len"] == len(w["core"]), name


def test_host_form_is_the_python_rule():
    assert len(HOST) > 300
    for n, g in zip(HOST, host_results()):
        _host_same(n, g, S.want(ROW[n]))


def test_it_is_the_host_side_chain_over_the_carrying_entry_point():
    """The rule run from the host, one satmi_cdcl_carry_batch_host call per round of trials over
    the instances that still have one: the same status, final core, kept lemmas and counters."""
    B = len(HOST)
    f, carry = [ROW[n][1] for n in HOST], [ROW[n][3] for n in HOST]
    state = [dict(status=None, W=None, p=0, kept=c, total=None, done=False, a=list(ROW[n][2])) for n, c in zip(HOST, carry)]
    rounds = 0
    while not all(s["done"] for s in state):
        live = [b for b in range(B) if not state[b]["done"]]
        res = cdcl_sound.cdcl_carry_batch([f[b] for b in live], [state[b]["a"] for b in live], [state[b]["kept"] for b in live])
        for b, r in zip(live, res):
            s, c = state[b], [r["counters"][k] for k in S.COUNTERS]
            s["total"] = c if s["total"] is None else \
                [max(x, y) if i == S.MAX_LEVEL else x + y for i, (x, y) in enumerate(zip(s["total"], c))]
            s["kept"], st = r["kept"], r["status"]
            if s["W"] is None:      # query 0
                s["status"], s["W"] = st, list(r["core"] or [])
                s["done"] = st != S.ASSUMED
            elif st == S.ASSUMED:
                s["W"] = [x for x in s["a"] if x in r["core"]]
            elif st in (S.SAT, S.LIMIT):
                s["p"] += 1
            else:
                s["status"], s["W"], s["done"] = st, [], True
            if not s["done"]:
                s["done"] = s["p"] >= len(s["W"])
                s["a"] = s["W"][:s["p"]] + s["W"][s["p"] + 1:]
        rounds += 1
    assert rounds == max(g["shrink"]["queries"] for g in host_results()) >= 6
    for n, g, s in zip(HOST, host_results(), state):
        assert (g["status"], g["core"] or [], g["kept"]) == (s["status"], s["W"], s["kept"]), n
        assert [g["counters"][k] for k in S.COUNTERS] == s["total"], n


def test_a_small_first_room_runs_again_to_the_same_answer():
    """The rows that end FULL in their room on the device form, and others, in a first room of two
    words: the host form runs them again from the input carry with four times the room."""
    names = ["full in a trial", "full at the closing record", "hand row", "carry in", "70 selectors, a chain", "unsat trial"]
    assert [S.want(ROW[n])["status"] for n in names[:2]] == [S.FULL, S.FULL]
    cdcl_sound.debug_room(2)
    try:
        res = cdcl_sound.cdcl_shrink_batch([ROW[n][1] for n in names], [ROW[n][2] for n in names],
                                           [ROW[n][3] for n in names], room=(2, 2), kept_room=(1, 1))
    finally:
        cdcl_sound.debug_room(0)
    for n, r in zip(names, res):
        _host_same(n, r, S.solve(ROW[n][1], ROW[n][2], 0, ROW[n][3]))
    assert [r["status"] for r in res[:2]] == [S.ASSUMED, S.ASSUMED]


def test_answers_pass_the_checkers_and_the_cores_are_minimal():
    """Every ASSUMED answer's (formula + core units, proof) is PROVEN by the refutation check and
    survives the trim; the same proof against the core less one literal is not; and under the
    core less any one literal the carrying entry point answers SAT with a model the model check
    accepts."""
    got = [(n, g) for n, g in zip(HOST, host_results()) if g["status"] == S.ASSUMED]
    assert len(got) > 200 and all(g["shrink"]["limit_trials"] == 0 for _, g in got)
    pairs = [refute.proof_of_cdcl_assumed(ROW[n][1], g) for n, g in got]
    chk = refute.check_refutations([p[0] for p in pairs], [p[1] for p in pairs])
    trm = refute.trim_refutations([p[0] for p in pairs], [p[1] for p in pairs])
    for (n, _), c, t in zip(got, chk, trm):
        assert c["proven"] and t["proven"], n
    assert refute.check_refutation(*pairs[0])
    less = [(n, g, x) for n, g in got for x in g["core"]]
    fs = [ROW[n][1] + _units([y for y in g["core"] if y != x]) for n, g, x in less]
    chk = refute.check_refutations(fs, [g["proof"] for _, g, _ in less])
    assert not any(c["proven"] for c in chk)
    res = cdcl_sound.cdcl_carry_batch([ROW[n][1] for n, _, _ in less], [[y for y in g["core"] if y != x] for n, g, x in less],
                                      [g["kept"] for _, g, _ in less])
    assert all(r["status"] == S.SAT for r in res)
    ok = check.check_models(fs, [[r["model"]] for r in res])
    assert all(m[0]["ok"] for m in ok)
    unsat = [(n, g) for n, g in zip(HOST, host_results()) if n == "unsat trial"]
    assert unsat[0][1]["status"] == S.UNSAT and unsat[0][1]["core"] == []
    assert refute.check_refutation(ROW["unsat trial"][1], unsat[0][1]["proof"])


def test_solver_and_solve_with_minimal_core():
    f, a = S.HAND
    with incremental.Solver(bootstrap_with=f) as s:
        assert s.solve(assumptions=a) is False and s.get_core() == [3, 2, 1]
        assert "trials" not in s.accum_stats()
        assert s.solve(assumptions=a, minimal_core=True) is False and s.get_core() == [3, 2]
        formula, proof = s.get_proof()
        assert formula == f + _units([3, 2]) and refute.check_refutation(formula, proof)
        assert not refute.check_refutation(f + _units([3]), proof) and s.nof_lemmas() == len(proof) - 1
        st = s.accum_stats()
        assert st["queries"] == 2 and 1 <= st["trials"] <= 3
        assert s.solve(assumptions=[1, 3], minimal_core=True) is True and s.get_core() is None
        assert R.satisfies(f + _units([1, 3]), s.get_model())
    for idle in (0, 2):
        f, a = S.php_groups_row(idle)
        with incremental.Solver(bootstrap_with=f) as s:
            assert s.solve(assumptions=a, minimal_core=True) is False
            assert s.get_core() == S.solve(f, a)["core"] and sorted(s.get_core()) == S.A.SELECTORS
            assert refute.check_refutation(*s.get_proof()) and s.accum_stats()["trials"] == 6
        sat, model, proof, core = solvers.cdcl_sound_solve(f, a, minimal_core=True)
        assert sat is False and model is None and core == S.solve(f, a)["core"]
        assert refute.check_refutation(f + _units(core), proof)
    f, a = S.HAND
    assert solvers.cdcl_sound_solve(f, a, minimal_core=True)[3] == [3, 2]
    # with the keyword False, today's answers
    assert solvers.cdcl_sound_solve(f, a)[3] == [3, 2, 1] == solvers.cdcl_sound_solve(f, a, minimal_core=False)[3]
    assert solvers.cdcl_sound_solve(f, None, minimal_core=True) == solvers.cdcl_sound_solve(f)
    f, a = S.unsat_trial_row()
    sat, _, proof, core = solvers.cdcl_sound_solve(f, a, minimal_core=True)
    assert sat is False and core == [] and refute.check_refutation(f, proof)
