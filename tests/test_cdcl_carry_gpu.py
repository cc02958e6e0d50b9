"""GPU checks of the sound CDCL with carried lemmas (csrc/cdcl_sound.hip's carrying kernel, its
pack and its host form) at the rows of tests/cdcl_carry_rows.py: the kernel is the Python rule
exactly -- status, counters, model row, core, info, carry_out and the region's words -- in both
clause forms and on a one-wave grid; with nothing carried it is the assumption-carrying entry
point word for word; a chain of queries runs in place on one stream; a malformed carry is
refused with its region untouched; the answers pass the library's own checkers."""
import functools

import numpy as np
import pytest

import cdcl_assume_rows as A
import cdcl_carry_rows as C
import cdcl_sound_rows as R
from satmi import _capi, cdcl_sound, incremental, refute, solvers
from satmi.cnf import pack

pytestmark = pytest.mark.gpu

GUARD, NG = 0x5A5A5A5A, 8
ROWS = C.rows()
NAMES = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}
SHORT = [n for n in NAMES if max([len(c) for c in ROW[n][1]] + [0]) <= R.SHORT_MAX and n != "sparse ids"]


def _units(lits):
    return [[l] for l in lits]


@functools.lru_cache(maxsize=None)
def want(name):
    _, f, a, c, room, nv = ROW[name]
    return C.solve(f, a, C.LIMITS.get(name, 0), c, room, nv)


def spec(f, a=(), carry=(), room=None, nv=None, words=None, carry_in=None, limit=0):
    """One instance of a launch: `words` = what lies in its region before (default: the carried
    records, cut at the room), `carry_in` = (records, words) (default: those of `carry`), `room`
    = the region's words (default: what the rule needs)."""
    f, a, carry = [list(c) for c in f], list(a), [list(c) for c in carry]
    w = C.solve(f, a, limit, carry, room, nv)
    if room is None:
        room = max(w["words"], R.region_words(carry))
    if nv is None:
        nv = max([abs(l) for c in f + carry for l in c] + [abs(l) for l in a] + [0])
    if words is None:
        words = C.records(carry)[:room]
    if carry_in is None:
        carry_in = (len(carry), R.region_words(carry))
    return dict(f=f, a=a, carry=carry, room=room, nv=nv, words=list(words), carry_in=tuple(carry_in), want=w)


def row_spec(name):
    _, f, a, c, room, nv = ROW[name]
    return spec(f, a, c, room, nv, limit=C.LIMITS.get(name, 0))


class Launch:
    """satmi_cdcl_carry_batch_device on torch tensors.  Every region is exactly its `room`, filled
    with guard words behind what lies there, and guard words lie behind the last region."""

    def __init__(self, specs, limit=0, grid=0, carry="given", short=False, core_stride=8, entry="carry"):
        import torch
        self.torch, self.specs = torch, specs
        self.dev = dev = torch.device("cuda", 0)
        self.B = B = len(specs)
        batch = pack([s["f"] for s in specs])
        begin, alits, _ = cdcl_sound.pack_assumptions([s["a"] for s in specs], B)
        self.nv = nv = max([s["nv"] for s in specs] + [0])
        self.mlen = mlen = max([len(c) for s in specs for c in s["f"]] + [0])
        assert not short or 1 <= mlen <= R.SHORT_MAX
        self.lb = lb = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([s["room"] for s in specs], out=lb[1:])
        region = np.full(int(lb[-1]) + NG, GUARD, dtype=np.int64)
        for b, s in enumerate(specs):
            assert len(s["words"]) <= s["room"]
            region[lb[b]:lb[b] + len(s["words"])] = s["words"]
        self.before = region.astype(np.int32)
        self.stride, self.cstride = max(nv, 1), core_stride
        cin = np.array([s["carry_in"] for s in specs], dtype=np.int64).reshape(B, 2)
        if carry == "zero":
            cin[:] = 0

        def up(a, dt=np.int32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

        def zeros(n, dt=torch.int32):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)

        self.t = [up(batch.inst_clause_begin), up(batch.clause_lit_begin), up(batch.lits)]
        self.d_nv, self.d_lb = up([s["nv"] for s in specs]), up(lb, np.int64)
        self.d_ab, self.d_al = up(begin), up(alits)
        self.lemmas = up(self.before)
        self.status, self.counters = zeros(B), zeros(B * 8, torch.int64)
        self.row_len, self.row_lits = zeros(B), zeros(B * self.stride)
        self.core_len = zeros(B)
        self.core_lits = torch.full((B * core_stride + NG,), GUARD, dtype=torch.int32, device=dev)
        self.info = zeros(B * 4, torch.int64)
        self.carry = torch.cat([up(cin.reshape(-1), np.int64), torch.full((NG,), GUARD, dtype=torch.int64, device=dev)])
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.solve(limit, grid, carry, entry)

    def solve(self, limit=0, grid=0, carry="given", entry="carry", d_ab=None, d_al=None):
        """One query, in place: carry_in and carry_out are the same array."""
        ptr = [x.data_ptr() for x in self.t]
        args = (self.B, *ptr, self.d_nv.data_ptr(), self.nv, self.mlen, self.lemmas.data_ptr(), self.d_lb.data_ptr(),
                self.status.data_ptr(), self.counters.data_ptr(), self.row_len.data_ptr(), self.row_lits.data_ptr(),
                self.stride, self.info.data_ptr(), (self.d_ab if d_ab is None else d_ab).data_ptr(), (self.d_al if d_al is None else d_al).data_ptr(),
                self.core_len.data_ptr(), self.core_lits.data_ptr(), self.cstride)
        cdcl_sound.debug_grid(grid, 1 if grid else 0)
        try:
            if entry == "assume":
                cdcl_sound.cdcl_assume_device(*args, conflict_limit=limit, stream=self.stream)
            else:
                cdcl_sound.cdcl_carry_device(*args, None if carry == "null" else self.carry.data_ptr(),
                                             self.carry.data_ptr(), conflict_limit=limit, stream=self.stream)
        finally:
            cdcl_sound.debug_grid(0, 0)

    def fetch(self):
        self.torch.cuda.current_stream(self.dev).synchronize()
        B = self.B
        o = {k: getattr(self, k).cpu().numpy() for k in
             ("lemmas", "status", "counters", "row_len", "row_lits", "core_len", "core_lits", "info", "carry")}
        o["counters"], o["info"] = o["counters"].reshape(B, 8), o["info"].reshape(B, 4)
        o["row_lits"] = o["row_lits"][:B * self.stride].reshape(B, self.stride)
        assert (o["core_lits"][B * self.cstride:] == GUARD).all() and (o["carry"][2 * B:] == GUARD).all()
        assert (o["lemmas"][self.lb[-1]:] == GUARD).all()
        o["core_lits"] = o["core_lits"][:B * self.cstride].reshape(B, self.cstride)
        o["carry"] = o["carry"][:2 * B].reshape(B, 2)
        return o

    def region(self, o, b):
        return o["lemmas"][self.lb[b]:self.lb[b + 1]].tolist()


def _same(name, L, o, b, w, carry_in, chained=False):
    """Instance b of a fetched launch against the rule's result `w` (`chained`: earlier queries
    wrote the region too, and their closing records may lie behind this one's last word)."""
    assert o["status"][b] == w["status"], name
    assert o["counters"][b].tolist() == w["counters"], name
    model = w["model"] or []
    assert o["row_len"][b] == len(model) and o["row_lits"][b, :len(model)].tolist() == model, name
    core = (w["core"] or []) if w["status"] == C.ASSUMED else []
    k = min(len(core), L.cstride)
    assert o["core_len"][b] == len(core) and o["core_lits"][b, :k].tolist() == core[:k], name
    assert o["info"][b, :3].tolist() == [w["records"], w["words"], w["flags"]], name
    before = L.before[L.lb[b]:L.lb[b + 1]].tolist()
    if w["status"] == C.TOO_LARGE:       # untouched; its input back, or nothing of a bad carry
        assert L.region(o, b) == before, name
        assert o["carry"][b].tolist() == ([0, 0] if w["flags"] & C.BAD_CARRY else list(carry_in)), name
        return
    rec = C.records(w["lemmas"])
    assert L.region(o, b)[:len(rec)] == rec and (chained or L.region(o, b)[len(rec):] == before[len(rec):]), name
    assert o["carry"][b].tolist() == [len(w["kept"]), R.region_words(w["kept"])], name


def test_rows_reach_every_path_on_the_cpu():
    assert {want(n)["status"] for n in NAMES if ROW[n][3]} == {C.SAT, C.UNSAT, C.ASSUMED, C.LIMIT, C.FULL, C.TOO_LARGE}
    for hit in C.HITS:
        assert any(want(n)["hits"][hit] for n in NAMES), hit
    assert len(SHORT) > 100 and "long clause" not in SHORT and "carried lemma of 65" in SHORT


@pytest.mark.parametrize("group,grid", [("all", 0), ("short", 0), ("short", 1)])
def test_kernel_is_the_python_rule(group, grid):
    """Every row, in the wave-per-clause form ("all": a 300-literal clause is among them), the
    lane-per-clause form ("short"), and with one wave taking every formula in turn (grid 1 x 1):
    consecutive instances with different carries then share the wave's LDS."""
    for limit in sorted(set(C.LIMITS.values()) | {0}):
        names = [n for n in (NAMES if group == "all" else SHORT) if C.LIMITS.get(n, 0) == limit]
        if limit:      # (a neighbour, so the one-wave grid has two instances here too)
            names = names + ["carried unit at level 0"]
        specs = [row_spec(n) if C.LIMITS.get(n, 0) == limit else
                 spec(*ROW[n][1:6], limit=limit) for n in names]
        L = Launch(specs, limit=limit, grid=grid, short=group == "short")
        o = L.fetch()
        for b, (n, s) in enumerate(zip(names, specs)):
            _same(n, L, o, b, s["want"], s["carry_in"])


@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_record_sizes_at_the_wave_step_boundaries(k):
    """A carry of exactly one record of k literals: unit after one round; and the same record
    behind another, falsified at level 0."""
    f, a, carry = C.wide_carry_row(k)
    refuted = [[-v] for v in range(1, k + 1)]
    specs = [spec(f, a, carry), spec(refuted, [], [[k + 1, -(k + 1)]] + carry), spec(refuted, [], carry)]
    assert [s["want"]["status"] for s in specs] == [C.SAT, C.UNSAT, C.UNSAT]
    assert specs[0]["carry_in"] == (1, k + 1) and specs[2]["want"]["hits"][C.HITS[4]] == 1
    L = Launch(specs)
    o = L.fetch()
    for b, s in enumerate(specs):
        _same(f"record of {k}, instance {b}", L, o, b, s["want"], s["carry_in"])


@pytest.mark.parametrize("carry", ["null", "zero"])
def test_without_a_carry_every_output_is_the_assumption_entry_points(carry):
    """The rows of cdcl_assume_rows with a NULL carry_in and with an all-zero one, against
    satmi_cdcl_assume_batch_device on the same arrays: word for word."""
    rows = [r for r in A.rows() if r[0] != "sparse ids"]
    specs = [spec(f, a) for _, f, a in rows]
    old, new = Launch(specs, entry="assume"), Launch(specs, carry=carry)
    o, n = old.fetch(), new.fetch()
    for k in ("lemmas", "status", "counters", "row_len", "row_lits", "core_len", "core_lits", "info"):
        assert np.array_equal(o[k], n[k]), k
    assert n["carry"].tolist() == [[len(s["want"]["kept"]), R.region_words(s["want"]["kept"])] for s in specs]
    assert {C.SAT, C.UNSAT, C.ASSUMED} <= set(n["status"].tolist())


CHAIN_F = [A.php_selector_row()[0], R.php(4), R.random_row()[3], [[1, 2], [-1, 2]], R.php(3)]
CHAIN_A = [[[20] + A.SELECTORS[:5], [1, 6], [3, -7], [-2], [1]],
           [A.SELECTORS[:3] + [21], [11, 16], [-3], [1], [4, 2]],
           [A.php_selector_row()[1], [2, 7, 12], [5, 9, -11], [-2, 1], []]]


def test_device_chain_in_place_on_one_stream():
    """Three queries on the same regions with carry_in == carry_out and no host copy between
    them equal the rule's chain; the existing pack, check and trim then certify the last."""
    import torch
    B = len(CHAIN_F)
    chains = [C.chain([(f, CHAIN_A[q][b]) for q in range(3)]) for b, f in enumerate(CHAIN_F)]
    last = [c[-1] for c in chains]
    assert {C.UNSAT, C.ASSUMED} <= {w["status"] for w in last} and any(c[1]["hits"][C.HITS[2]] for c in chains)
    specs = [spec(f, CHAIN_A[0][b], room=max(w["words"] for w in chains[b]),
                  nv=max(abs(l) for c in f for l in c) + 22) for b, f in enumerate(CHAIN_F)]
    L = Launch(specs, core_stride=10)
    later = []
    for q in (1, 2):        # (the assumption arrays of the later queries are uploaded before the first is read)
        begin, alits, _ = cdcl_sound.pack_assumptions(CHAIN_A[q], B)
        later.append((torch.from_numpy(begin).to(L.dev), torch.from_numpy(alits).to(L.dev)))
    for d_ab, d_al in later:
        L.solve(d_ab=d_ab, d_al=d_al)
    # the pack of the assumption-carrying solve reads the region as it is
    ccap = sum(len(w["lemmas"]) for w in last if w["status"] in (C.UNSAT, C.ASSUMED))
    lcap = sum(len(c) for w in last if w["status"] in (C.UNSAT, C.ASSUMED) for c in w["lemmas"])
    pib = torch.zeros(B + 1, dtype=torch.int32, device=L.dev)
    pcb = torch.full((ccap + 1 + NG,), GUARD, dtype=torch.int32, device=L.dev)
    plits = torch.full((lcap + NG,), GUARD, dtype=torch.int32, device=L.dev)
    totals = torch.zeros(2, dtype=torch.int64, device=L.dev)
    cdcl_sound.assume_pack_device(B, L.status.data_ptr(), L.lemmas.data_ptr(), L.d_lb.data_ptr(), L.info.data_ptr(),
                                  pib.data_ptr(), pcb.data_ptr(), ccap, plits.data_ptr(), lcap, totals.data_ptr(),
                                  stream=L.stream)
    o = L.fetch()
    for b, w in enumerate(last):
        _same(f"chain {b}", L, o, b, w, None, chained=True)
    assert totals.tolist() == [ccap, lcap]
    assert (pcb[ccap + 1:] == GUARD).all() and (plits[lcap:] == GUARD).all()
    # against F plus the core: PROVEN by the check and by the trim; against F alone not where the core is needed
    cores = [w["core"] or [] for w in last]
    out = {}
    for key, fs in (("core", [f + _units(c) for f, c in zip(CHAIN_F, cores)]), ("alone", CHAIN_F)):
        batch = pack(fs)
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(L.dev) for x in
             (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits)]
        chk = torch.zeros(B * 4, dtype=torch.int32, device=L.dev)
        trm = torch.zeros(B * 6, dtype=torch.int32, device=L.dev)
        cmark = torch.zeros(len(batch.clause_lit_begin), dtype=torch.int32, device=L.dev)
        lmark = torch.zeros(ccap + 1, dtype=torch.int32, device=L.dev)
        ptr = [x.data_ptr() for x in t]
        refute.check_refutations_device(B, *ptr, pib.data_ptr(), pcb.data_ptr(), plits.data_ptr(), L.nv, 0,
                                        chk.data_ptr(), None, L.stream)
        refute.trim_refutations_device(B, *ptr, pib.data_ptr(), pcb.data_ptr(), plits.data_ptr(), L.nv, 0,
                                       trm.data_ptr(), cmark.data_ptr(), lmark.data_ptr(), L.stream)
        torch.cuda.current_stream(L.dev).synchronize()
        out[key] = (chk.cpu().numpy().reshape(B, 4)[:, 0], trm.cpu().numpy().reshape(B, 6)[:, 0])
    needed = 0
    for b, w in enumerate(last):
        if w["status"] in (C.UNSAT, C.ASSUMED):
            assert out["core"][0][b] == _capi.REFUTE_PROVEN and out["core"][1][b] == _capi.REFUTE_PROVEN, b
            if w["core"] and A.solve(CHAIN_F[b])["status"] == A.SAT:
                assert out["alone"][0][b] != _capi.REFUTE_PROVEN and out["alone"][1][b] != _capi.REFUTE_PROVEN, b
                needed += 1
        else:
            assert out["core"][0][b] == _capi.REFUTE_OPEN, b
    assert needed >= 1


def test_room_equal_to_the_carried_words():
    """An instance that needs no lemma ends SAT; one that needs one ends FULL with carry_out ==
    carry_in and its carried words unchanged."""
    names = ["room equal to the carry: SAT", "room equal to the carry: FULL", "room one short of the closing record"]
    specs = [row_spec(n) for n in names]
    assert [s["room"] for s in specs] == [R.region_words(s["carry"]) for s in specs]
    L = Launch(specs)
    o = L.fetch()
    assert o["status"].tolist() == [C.SAT, C.FULL, C.FULL]
    for b, s in enumerate(specs):
        _same(names[b], L, o, b, s["want"], s["carry_in"])
        assert o["carry"][b].tolist() == list(s["carry_in"]) and L.region(o, b) == C.records(s["carry"])
    assert o["info"][1:, 2].tolist() == [C.TRUNCATED, C.TRUNCATED]


PHP3_KEPT = C.solve(R.php(3))["kept"]
RAW = C.records(PHP3_KEPT)        # six records, 18 words
MALFORMED = {       # kind -> (region words, (records, words), room)
    "negative records": (RAW, (-1, len(RAW)), len(RAW) + 8),
    "negative words": (RAW, (6, -1), len(RAW) + 8),
    "words exceed the room": (RAW[:10], (6, len(RAW)), 10),
    "record of length 0": (RAW[:3] + [0] + RAW[3:], (7, len(RAW) + 1), len(RAW) + 8),
    "record of negative length": ([-2] + RAW, (7, len(RAW) + 1), len(RAW) + 8),
    "record runs past the words": (RAW, (6, len(RAW) - 1), len(RAW) + 8),
    "chain ends before the words": (RAW, (6, len(RAW) + 1), len(RAW) + 8),
    "fewer records than stated": (RAW, (7, len(RAW)), len(RAW) + 8),
    "more records than stated": (RAW, (5, len(RAW)), len(RAW) + 8),
    "literal 0": (RAW[:4] + [0] + RAW[5:], (6, len(RAW)), len(RAW) + 8),
    "literal INT32_MIN": (RAW[:4] + [C.I32_MIN] + RAW[5:], (6, len(RAW)), len(RAW) + 8),
    "literal beyond inst_nvars": (RAW[:4] + [13] + RAW[5:], (6, len(RAW)), len(RAW) + 8),
    "literal beyond inst_nvars, negative": (RAW[:4] + [-13] + RAW[5:], (6, len(RAW)), len(RAW) + 8),
}


def test_malformed_carries_are_refused_beside_untouched_neighbours():
    """One instance for each kind, each between two neighbours: TOO_LARGE with BAD_CARRY, the
    region's words unchanged, carry_out (0, 0); the neighbours as without them."""
    assert RAW[0] >= 1 and RAW[4] != 0 and len(PHP3_KEPT) == 6
    good = [spec(R.php(3), [], PHP3_KEPT), spec(R.php(3), [2], PHP3_KEPT[:2])]
    specs, kinds = [good[0]], []
    for kind, (words, cin, room) in MALFORMED.items():
        s = spec(R.php(3), [], [], room=room, nv=12, words=words, carry_in=cin)
        s["want"] = dict(s["want"], status=C.TOO_LARGE, flags=C.BAD_CARRY, records=0, words=0, model=None, core=None,
                         counters=[0] * 8, kept=[], lemmas=[])
        specs += [s, good[len(specs) // 2 % 2]]
        kinds.append(kind)
    L = Launch(specs, grid=1)       # one wave takes them in turn: nothing of a refused instance stays behind
    o = L.fetch()
    alone = Launch(good)
    a = alone.fetch()
    for b, s in enumerate(specs):
        if b % 2:
            _same(kinds[b // 2], L, o, b, s["want"], s["carry_in"])
            assert o["info"][b, 2] == C.BAD_CARRY and L.region(o, b) == L.before[L.lb[b]:L.lb[b + 1]].tolist()
        else:
            g = good.index(s)
            _same(f"neighbour {b}", L, o, b, s["want"], s["carry_in"])
            for k in ("status", "counters", "row_len", "row_lits", "core_len", "info", "carry"):
                assert np.array_equal(o[k][b], a[k][g]), (b, k)
            assert L.region(o, b) == alone.region(a, g)


def test_carry_pack_fits_and_one_short_on_each_capacity():
    import torch
    names = ["php 4 resumed after 4 conflicts", "carried lemma of 65", "room equal to the carry: FULL",
             "bogus: carried literal beyond inst_nvars", "php 3 five selectors with the six's lemmas",
             "carried clause over a new variable"]
    specs = [row_spec(n) for n in names]
    L = Launch(specs)
    o = L.fetch()
    kept = [s["want"]["kept"] for s in specs]
    assert kept[3] == [] and {s["want"]["status"] for s in specs} >= {C.UNSAT, C.SAT, C.FULL, C.TOO_LARGE}
    tn, tl = sum(map(len, kept)), sum(len(c) for k in kept for c in k)
    B = len(specs)
    for ccap, lcap in ((tn, tl), (tn - 1, tl), (tn, tl - 1)):
        kib = torch.full((B + 1 + NG,), GUARD, dtype=torch.int32, device=L.dev)
        kcb = torch.full((ccap + 1 + NG,), GUARD, dtype=torch.int32, device=L.dev)
        klits = torch.full((lcap + NG,), GUARD, dtype=torch.int32, device=L.dev)
        totals = torch.zeros(2, dtype=torch.int64, device=L.dev)
        cdcl_sound.carry_pack_device(B, L.lemmas.data_ptr(), L.d_lb.data_ptr(), L.carry.data_ptr(), kib.data_ptr(),
                                     kcb.data_ptr(), ccap, klits.data_ptr(), lcap, totals.data_ptr(), stream=L.stream)
        torch.cuda.current_stream(L.dev).synchronize()
        kib, kcb, klits = kib.cpu().numpy(), kcb.cpu().numpy(), klits.cpu().numpy()
        assert totals.tolist() == [tn, tl]
        assert (kib[B + 1:] == GUARD).all() and (kcb[ccap + 1:] == GUARD).all() and (klits[lcap:] == GUARD).all()
        if (ccap, lcap) == (tn, tl):
            got = [[klits[kcb[p]:kcb[p + 1]].tolist() for p in range(kib[b], kib[b + 1])] for b in range(B)]
            assert got == kept
        else:       # no instance has a lemma, and nothing else is written
            assert not kib[:B + 1].any() and kcb[0] == 0
            assert (kcb[1:ccap + 1] == GUARD).all() and (klits[:lcap] == GUARD).all()
    assert np.array_equal(L.fetch()["lemmas"], o["lemmas"])      # the pack reads the regions only


# ---- the host form
def _host_same(name, g, w):
    assert g["status"] == w["status"], name
    assert [g["counters"][k] for k in C.COUNTERS] == w["counters"], name
    assert g["model"] == w["model"] and g["kept"] == w["kept"], name
    assert (g["records"], g["region_words"], g["flags"]) == (w["records"], w["words"], w["flags"]), name
    if w["status"] in (C.UNSAT, C.ASSUMED):
        assert g["proof"] == w["lemmas"] and g["core"] == w["core"], name


HOST = [n for n in NAMES if ROW[n][4] is None and ROW[n][5] is None and n not in C.LIMITS]


@functools.lru_cache(maxsize=None)
def host_results():
    return cdcl_sound.cdcl_carry_batch([ROW[n][1] for n in HOST], [ROW[n][2] for n in HOST], [ROW[n][3] for n in HOST])


def test_host_form_is_the_python_rule():
    assert len(HOST) > 140
    for n, g in zip(HOST, host_results()):
        _host_same(n, g, want(n))


def test_a_small_first_room_runs_again_to_the_same_answer():
    names = ["php 4 resumed after 4 conflicts", "carried unit at level 0", "php 3 selectors resumed after 3 conflicts",
             "chain 0 query 1", "carried lemma of 65"]
    assert want(names[0])["words"] > R.region_words(ROW[names[0]][3]) + 8
    cdcl_sound.debug_room(2)
    try:
        res = cdcl_sound.cdcl_carry_batch([ROW[n][1] for n in names], [ROW[n][2] for n in names],
                                          [ROW[n][3] for n in names], room=(2, 2), kept_room=(1, 1))
    finally:
        cdcl_sound.debug_room(0)
    for n, r in zip(names, res):
        _host_same(n, r, want(n))


def test_grown_formula_and_a_bogus_lemma():
    """Solve F, add clauses, solve again with the kept lemmas: PROVEN against the grown formula.
    A bogus carried unit answers UNSAT, and the check fails at that lemma's index."""
    f = R.random_row()[5]
    first = cdcl_sound.cdcl_carry_batch([f], [[1, -2, 3]])[0]
    assert first["kept"] == C.solve(f, [1, -2, 3])["kept"] and first["kept"]
    grown = f + R.php(3)        # (over variables 1 .. 12 of f too)
    w = C.solve(grown, [], 0, first["kept"])
    r = cdcl_sound.cdcl_carry_batch([grown], None, [first["kept"]])[0]
    _host_same("grown", r, w)
    assert r["status"] == C.UNSAT and r["proof"][:len(first["kept"])] == first["kept"]
    assert refute.check_refutations([grown], [r["proof"]])[0]["proven"]
    _, bf, ba, bc, _, _ = ROW["bogus unit makes a satisfiable formula UNSAT"]
    good = [[2]]        # a lemma that does follow, in front of the bogus one
    r = cdcl_sound.cdcl_carry_batch([bf], [ba], [good + bc])[0]
    assert r["status"] == C.UNSAT and r["proof"] == good + bc + [[]]
    c = refute.check_refutations([bf], [r["proof"]], lemmas=True)[0]
    assert c["status"] == _capi.REFUTE_FAILED and c["first_failed"] == 1 and c["lemma_ok"][:2] == [1, 0]
    assert solvers.check_assignment(bf, cdcl_sound.cdcl_carry_batch([bf], [ba])[0]["model"])


def test_incremental_solver():
    f, a = A.php_selector_row()
    assert solvers.Solver is incremental.Solver
    with incremental.Solver(bootstrap_with=f) as s:
        assert s.nof_clauses() == len(f) and s.nof_lemmas() == 0 and s.get_model() is None
        assert s.solve(assumptions=[20, 21] + A.SELECTORS[:5]) is True       # a clause group switched off
        model = s.get_model()
        assert R.satisfies(f + _units([20, 21] + A.SELECTORS[:5]), model) and s.get_core() is None
        assert s.solve(assumptions=a) is False
        assert sorted(s.get_core()) == A.SELECTORS
        formula, proof = s.get_proof()
        assert formula == f + _units(s.get_core()) and refute.check_refutation(formula, proof)
        assert not refute.check_refutation(f, proof)
        lemmas = s.nof_lemmas()
        assert lemmas == len(proof) - 1 > 0
        s.add_clause([-A.SELECTORS[0]])       # the first group is gone for good
        assert s.solve(assumptions=A.SELECTORS[1:]) is True and s.nof_lemmas() >= lemmas
        assert s.solve(assumptions=A.SELECTORS) is False and s.get_core()[0] == A.SELECTORS[0]
        assert refute.check_refutation(*s.get_proof())
        st = s.accum_stats()
        assert st["queries"] == 4 and st["rounds"] > 4 and st["conflicts"] > 0
    # a search cut by conflict_limit returns None and then finishes, with the rule's slices
    with incremental.Solver(bootstrap_with=R.php(4)) as s:
        answers = []
        for _ in range(100):
            answers.append(s.solve(conflict_limit=8))
            if answers[-1] is not None:
                break
        last, slices = C.resume(R.php(4), (), 8)
        assert answers == [None] * (slices - 1) + [False] and slices >= 2
        formula, proof = s.get_proof()
        assert proof == last["lemmas"] and refute.check_refutation(formula, proof)
        assert s.accum_stats()["conflicts"] > 8
