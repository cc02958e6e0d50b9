"""GPU checks of the DPLL refutations (csrc/dpll.hip's logging kernels, csrc/dpll_proof.hip)
at the rows of tests/dpll_proof_rows.py: the logged search is the unlogged one, the log of
an UNSAT search is the post-order walk of its tree, and the refutation check proves it --
in the host form and in the device pipeline solve -> pack -> check on one stream."""
import functools

import numpy as np
import pytest

import oracle
import dpll_proof_rows as R
import refute_rows as rr
from satmi import _capi, solvers
from satmi.cnf import pack
from satmi.dpll import dpll_batch
from satmi.refute import (check_refutations, check_refutations_device, dpll_refutations, dpll_refutations_device,
                          dpll_refutations_packed, proof_of_dpll, trim_refutations)

pytestmark = pytest.mark.gpu

CTRS = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")
ROWS = R.all_rows()
NAMES = [n for n, _ in ROWS]
FORMULA = dict(ROWS)


def _small(name):
    return name.startswith(("mixed", "hand"))


# Batches by the kernel the default policy gives them: the clause kernel with incremental
# rounds (lengths 1 .. 4), the fixed kernel of the bench class (3-SAT, n <= 100), the general
# kernel's LDS form (an empty clause; a clause of 72 literals) and its wide form (300 literals).
GROUPS = {
    "inc": [n for n in NAMES if _small(n) and n != "hand0"],
    "fixed": [n for n in NAMES if n.startswith(("ksat", "bench"))],
    "lds": ["hand0", "deep", "hand1", "mixed0"],
    "wide": ["long", "hand4", "hand5", "mixed1"],
}


@functools.lru_cache(maxsize=None)
def want(name):
    return oracle.dpll(FORMULA[name], "sound", max_solutions=1, sol_cap=1)


def _unsat(name):
    o = want(name)
    return o["status"] == 0 and o["counters"]["solutions"] == 0


@functools.lru_cache(maxsize=None)
def logged(group):
    """The host form on the group's rows in one call: name -> dpll_refutations dict."""
    return dict(zip(GROUPS[group], dpll_refutations([FORMULA[n] for n in GROUPS[group]])))


@functools.lru_cache(maxsize=None)
def unlogged(group, policy):
    _capi.set_kernel(policy)
    try:
        return dpll_batch([FORMULA[n] for n in GROUPS[group]], mode="sound", max_solutions=1)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)


def every_logged():
    out = {}
    for g in GROUPS:
        out.update(logged(g))
    return out


@pytest.mark.parametrize("group", list(GROUPS))
def test_logged_search_is_the_unlogged_search(group):
    """Status, counters (ticks excepted), model and root assignment: the logging kernel, the
    general kernel, whatever kernel the default policy takes, and the oracle."""
    names = GROUPS[group]
    if group == "fixed":
        assert _capi.plan(100, 426, 1278, 3)[0] == _capi.KERNEL_INC and _capi.scan_shape(100, 426, 3)[3]
    got = logged(group)
    # (pinned, the general kernel's LDS form does not hold the 300-literal clause)
    general = unlogged(group, _capi.KERNEL_WIDE if group == "wide" else _capi.KERNEL_GENERAL)
    default = unlogged(group, _capi.KERNEL_AUTO)
    for b, n in enumerate(names):
        r, o = got[n], want(n)
        for other in (general, default):
            assert r["status"] == int(other.status[b]), n
            assert r["counters"] == other.counter_dict(b), n
            assert (r["model"] is None and other.num_solutions(b) == 0) or [r["model"]] == other.solutions(b), n
            assert r["root"] == other.root_assignment(b), n
        assert r["status"] == o["status"], n
        assert {k: r["counters"][k] for k in CTRS} == {k: o["counters"][k] for k in CTRS}, n
        assert ([r["model"]] if r["model"] is not None else []) == o["solutions"][:1], n
        assert r["root"] == o["root_assign"], n
        assert r["sat"] == (not _unsat(n)), n


@pytest.mark.parametrize("group", list(GROUPS))
def test_unsat_rows_log_the_postorder_walk_and_the_check_proves_it(group):
    names = [n for n in GROUPS[group] if _unsat(n)]
    assert names
    got = logged(group)
    default = unlogged(group, _capi.KERNEL_AUTO)
    proofs = [proof_of_dpll(got[n]) for n in names]
    for n, p in zip(names, proofs):
        c = default.counter_dict(GROUPS[group].index(n))
        assert got[n]["lemmas"] == len(p) == c["decisions"] + 1, n
        assert c["conflicts"] == c["decisions"] // 2 + 1, n
        assert got[n]["log_words"] == len(p) + sum(map(len, p)), n
        assert R.is_postorder(p), n
    formulas = [FORMULA[n] for n in names]
    checked = check_refutations(formulas, proofs, lemmas=True)
    trimmed = trim_refutations(formulas, proofs)
    cores = [[f[c] for c in t["core"]] for f, t in zip(formulas, trimmed)]
    again = check_refutations(cores, [t["proof"] for t in trimmed])
    for n, f, p, c, t, a in zip(names, formulas, proofs, checked, trimmed, again):
        assert c["proven"] and c["failed"] == 0 and c["first_failed"] == -1, n
        assert c["lemma_ok"] == [1] * len(p), n
        assert t["proven"] and t["failed"] == 0 and t["proof"][-1] == [], n
        assert a["proven"] and a["failed"] == 0, n
        nv = rr.max_vars_of(f)
        if nv <= 14:
            words, ok = rr.evaluate(f, p)
            assert words == [rr.PROVEN, 0, -1, c["flags"]] and ok == c["lemma_ok"], n
            assert R.satisfiable(f, nv) is None, n


def test_sat_rows_have_no_lemma_and_stay_open():
    got = every_logged()
    names = [n for n in got if not _unsat(n)]
    assert len(names) >= 20
    for n in names:
        assert got[n]["sat"] is True and got[n]["proof"] is None, n
        with pytest.raises(ValueError):
            proof_of_dpll(got[n])
    _, proof, info = dpll_refutations_packed(pack([FORMULA[n] for n in names]))
    assert int(proof.inst_clause_begin[-1]) == 0 and (np.diff(proof.inst_clause_begin) == 0).all()
    assert (info[:, 0] > 0).any()                       # some SAT searches closed subtrees on the way
    for c in check_refutations([FORMULA[n] for n in names], proof):
        assert c["status"] == _capi.REFUTE_OPEN and c["failed"] == 0, c


def test_a_proof_fails_against_a_satisfiable_weakening():
    """Soundness at size: the row minus one clause of its trimmed core, where that is
    satisfiable (the model is exhibited here), does not carry the row's proof."""
    got = logged("inc")
    names = [n for n in GROUPS["inc"] if n.startswith("mixed") and _unsat(n) and got[n]["counters"]["decisions"] > 0
             and rr.max_vars_of(FORMULA[n]) <= 12]
    formulas = [FORMULA[n] for n in names]
    proofs = [got[n]["proof"] for n in names]
    weak, carried = [], []
    for f, p, t in zip(formulas, proofs, trim_refutations(formulas, proofs)):
        for c in t["core"]:
            g = f[:c] + f[c + 1:]
            model = R.satisfiable(g, 12)
            if model is not None:
                assert all(any(l in model for l in cl) for cl in g)
                weak.append(g)
                carried.append(p)
                break
    assert len(weak) >= 10
    for c in check_refutations(weak, carried):
        assert c["status"] == _capi.REFUTE_FAILED and c["failed"] >= 1


# ---- the device pipeline
NG, GUARD = 64, 0x5A5A5A5A


class Pipeline:
    """satmi_dpll_refutations_device -> satmi_check_refutations_device on one stream, on torch
    tensors with guard words around the proof arrays."""

    def __init__(self, formulas, room, ccap, lcap):
        import torch
        dev = torch.device("cuda", 0)
        batch = pack(formulas)
        B = self.B = batch.num_instances
        nv, mc, ml = batch.maxima()
        lens = np.diff(batch.clause_lit_begin[:int(batch.inst_clause_begin[B]) + 1])
        mlen = int(lens.max(initial=0)) if (lens.min(initial=1) >= 1 or lens.max(initial=0) > 5) else 0
        stride = max(1, nv)

        def up(a, dt=np.int32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

        def zeros(n, dt=torch.int32):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)
        t = [up(a) for a in (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits, batch.inst_nvars)]
        room = np.broadcast_to(np.asarray(room, dtype=np.int64), (B,))
        lb = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
        self.log = torch.full((int(lb[-1]) + NG,), GUARD, dtype=torch.int32, device=dev)
        self.lb = lb
        d_lb = up(lb, np.int64)
        self.status, self.counters = zeros(B), zeros(B * 8, torch.int64)
        sol_len, sol_lits, root_len, root_lits = zeros(B), zeros(B * stride), zeros(B), zeros(B * stride)
        self.pib = zeros(B + 1)
        self.pcb = torch.full((ccap + 1 + NG,), GUARD, dtype=torch.int32, device=dev)
        self.plits = torch.full((lcap + NG,), GUARD, dtype=torch.int32, device=dev)
        self.info, self.totals = zeros(B * 4, torch.int64), zeros(2, torch.int64)
        self.out = zeros(B * 4)
        s = torch.cuda.current_stream(dev)
        dpll_refutations_device(B, *(x.data_ptr() for x in t), nv, mc, ml, mlen, self.status.data_ptr(),
                                self.counters.data_ptr(), sol_len.data_ptr(), sol_lits.data_ptr(),
                                root_len.data_ptr(), root_lits.data_ptr(), 1, stride, self.log.data_ptr(),
                                d_lb.data_ptr(), self.pib.data_ptr(), self.pcb.data_ptr(), ccap,
                                self.plits.data_ptr(), lcap, self.info.data_ptr(), self.totals.data_ptr(),
                                stream=s.cuda_stream)
        # (max_clause_len 0: the check's wave-per-clause form, whatever the lemmas' lengths)
        check_refutations_device(B, *(x.data_ptr() for x in t[:3]), self.pib.data_ptr(), self.pcb.data_ptr(),
                                 self.plits.data_ptr(), nv, 0, self.out.data_ptr(), None, s.cuda_stream)
        s.synchronize()
        self.h = {k: getattr(self, k).cpu().numpy() for k in ("status", "counters", "pib", "pcb", "plits", "info",
                                                              "totals", "out", "log")}
        self.h["info"] = self.h["info"].reshape(B, 4)
        self.h["out"] = self.h["out"].reshape(B, 4)
        self.h["counters"] = self.h["counters"].reshape(B, 8)
        self.ccap, self.lcap = ccap, lcap

    def proof(self, b):
        pib, pcb, plits = self.h["pib"], self.h["pcb"], self.h["plits"]
        return [plits[pcb[c]:pcb[c + 1]].tolist() for c in range(pib[b], pib[b + 1])]

    def raw_log(self, b):
        """The records instance b's region holds (all of them: only for a log that fitted)."""
        words = self.h["log"][self.lb[b]:self.lb[b] + self.h["info"][b, 1]]
        out, at = [], 0
        while at < len(words):
            out.append(words[at + 1:at + 1 + words[at]].tolist())
            at += 1 + words[at]
        return out

    def guards_intact(self):
        return ((self.h["pcb"][self.ccap + 1:] == GUARD).all() and (self.h["plits"][self.lcap:] == GUARD).all()
                and (self.h["log"][self.lb[-1]:] == GUARD).all())


@functools.lru_cache(maxsize=None)
def pipeline(group):
    return Pipeline([FORMULA[n] for n in GROUPS[group]], 1 << 16, 1 << 15, 1 << 19)


@pytest.mark.parametrize("group", list(GROUPS))
def test_device_pipeline_gives_the_host_forms_answers(group):
    p, got = pipeline(group), logged(group)
    assert p.guards_intact()
    assert int(p.h["totals"][0]) == int(p.h["pib"][-1]) == sum(len(r["proof"] or ()) for r in got.values())
    for b, n in enumerate(GROUPS[group]):
        r = got[n]
        assert int(p.h["status"][b]) == r["status"], n
        assert dict(zip(_capi.COUNTER_NAMES[:7], p.h["counters"][b].tolist())) == r["counters"], n
        assert p.h["info"][b, :3].tolist() == [r["lemmas"], r["log_words"], 0], n
        assert p.proof(b) == (r["proof"] or []), n
        want_out = [_capi.REFUTE_PROVEN, 0, -1, 0] if r["sat"] is False else [_capi.REFUTE_OPEN, 0, -1, 0]
        assert p.h["out"][b].tolist() == want_out, n


def test_a_sat_searchs_partial_log_closed_by_hand_fails():
    p = pipeline("fixed")
    picks = [b for b, n in enumerate(GROUPS["fixed"]) if not _unsat(n) and p.h["info"][b, 0] > 0]
    assert picks
    formulas = [FORMULA[GROUPS["fixed"][b]] for b in picks]
    partial = [p.raw_log(b) for b in picks]
    for b, lemmas in zip(picks, partial):
        assert len(lemmas) == p.h["info"][b, 0] and [] not in lemmas
    # what the search closed does follow; the formula has a model, so [] does not
    for c, lemmas in zip(check_refutations(formulas, [l + [[]] for l in partial], lemmas=True), partial):
        assert c["status"] == _capi.REFUTE_FAILED and c["failed"] == 1 and c["first_failed"] == len(lemmas)
        assert c["lemma_ok"] == [1] * len(lemmas) + [0]


def test_truncated_logs_are_flagged_counted_and_never_written_past():
    names = ["bench0", "ksat12", "ksat0", "deep", "hand1"]
    formulas = [FORMULA[n] for n in names]
    roomy = Pipeline(formulas, 1 << 16, 1 << 14, 1 << 18)
    need = roomy.h["info"][:, 1].copy()
    assert (roomy.h["info"][:, 2] == 0).all() and need[0] > 1000 and need[4] == 1
    # every region one word short of its need (a region of no word at all for [[1], [-1]])
    tight = Pipeline(formulas, np.maximum(need - 1, 0), 1 << 14, 1 << 18)
    assert tight.guards_intact()
    for b, n in enumerate(names):
        assert tight.h["info"][b, :3].tolist() == [roomy.h["info"][b, 0], need[b], 1 if need[b] else 0], n
        assert tight.proof(b) == [], n
        assert tight.h["out"][b, 0] == _capi.REFUTE_OPEN, n
    assert (tight.h["status"] == roomy.h["status"]).all()
    assert (tight.h["counters"][:, :7] == roomy.h["counters"][:, :7]).all()
    # what did fit is the roomy log's prefix, record by record
    b0 = int(roomy.lb[0])
    assert (tight.h["log"][:need[0] - 1][:500] == roomy.h["log"][b0:b0 + 500]).all()
    # the counted sizes, exactly: the proof the roomy call gave
    exact = Pipeline(formulas, need, 1 << 14, 1 << 18)
    assert (exact.h["info"] == roomy.h["info"]).all() and exact.guards_intact()
    for b in range(len(names)):
        assert exact.proof(b) == roomy.proof(b)
    assert (exact.h["out"] == roomy.h["out"]).all()


def test_proof_arrays_one_short_report_the_totals_and_stay_unwritten():
    names = ["ksat12", "deep", "hand1", "hand5"]
    formulas = [FORMULA[n] for n in names]
    roomy = Pipeline(formulas, 1 << 15, 1 << 12, 1 << 16)
    P, Lt = map(int, roomy.h["totals"])
    assert P == roomy.h["pib"][-1] > 100 and Lt == roomy.h["pcb"][P]
    for ccap, lcap in ((P - 1, Lt), (P, Lt - 1), (1, 1)):
        short = Pipeline(formulas, 1 << 15, ccap, lcap)
        assert short.h["totals"].tolist() == [P, Lt]
        assert (short.h["pib"] == 0).all() and short.h["pcb"][0] == 0
        assert (short.h["pcb"][1:] == GUARD).all() and (short.h["plits"] == GUARD).all()
        assert (short.h["out"][:, 0] == _capi.REFUTE_OPEN).all()
        assert (short.h["info"][:, :3] == roomy.h["info"][:, :3]).all()
    fit = Pipeline(formulas, 1 << 15, P, Lt)
    assert fit.guards_intact() and [fit.proof(b) for b in range(4)] == [roomy.proof(b) for b in range(4)]
    assert (fit.h["out"] == roomy.h["out"]).all()


def test_host_form_and_wrapper_reach_the_full_proof_on_their_own():
    names = ["bench1", "ksat13", "deep", "hand1", "hand5"]
    formulas = [FORMULA[n] for n in names]
    got = every_logged()
    L = _capi.load()
    try:
        for words in (1, 64):
            _capi.check(L.satmi_dpll_refutations_debug_room(words), "satmi_dpll_refutations_debug_room")
            for r, n in zip(dpll_refutations(formulas, room=(1, 1)), names):   # ... and 4x the room, again and again
                assert r == got[n], n
    finally:
        L.satmi_dpll_refutations_debug_room(0)
    assert L.satmi_dpll_refutations_debug_room(-1) == _capi.ERR_ARG


def test_all_rows_in_one_call_equal_the_rows_one_by_one():
    """One call over every row (the 300-literal clause takes the whole batch to the wide
    form) against one call per row (each in the form its own shape takes)."""
    whole = dpll_refutations([f for _, f in ROWS])
    grouped = every_logged()
    for (n, f), w in zip(ROWS, whole):
        one = dpll_refutations([f])[0]
        assert w == one == grouped[n], n


def test_deep_row_lemmas_past_64_literals_arrive_intact():
    r = logged("lds")["deep"]
    p = proof_of_dpll(r)
    k = R.DEEP_CHAIN
    assert R.tree_depth(p) == k - 1 > 64 and len(p) == 2 * (k - 1) + 1
    # the deepest conflict, then every False branch's conflict and the pop behind it
    assert p[0] == [-v for v in range(1, k)]
    assert p[1] == [-v for v in range(1, k - 1)] + [k - 1] and p[2] == [-v for v in range(1, k - 1)]
    assert p[-2:] == [[1], []]
    assert sum(len(c) > 64 for c in p) == 2 * (k - 1 - 64)   # per depth: the pop to it and the False conflict at it
    b = GROUPS["lds"].index("deep")
    assert pipeline("lds").h["out"][b].tolist() == [_capi.REFUTE_PROVEN, 0, -1, 0]   # wave-per-clause form
    assert check_refutations([FORMULA["deep"]], [p])[0]["proven"]


def test_long_row_goes_through_the_wide_form():
    f = FORMULA["long"]
    r = logged("wide")["long"]
    assert r["status"] == _capi.DPLL_EXHAUSTED and r["sat"] is False and r["counters"]["pure_assigns"] == 298
    assert check_refutations([f], [r["proof"]])[0]["proven"]
    # pinned to its LDS form the general kernel does not hold the clause: TOO_LARGE stays TOO_LARGE
    _capi.set_kernel(_capi.KERNEL_GENERAL)
    try:
        pinned = dpll_refutations([f, FORMULA["hand1"]])
        plain = dpll_batch([f, FORMULA["hand1"]], mode="sound", max_solutions=1)
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    assert pinned[0]["status"] == int(plain.status[0]) == _capi.DPLL_TOO_LARGE
    assert pinned[0]["proof"] is None and pinned[0]["lemmas"] == 0 and pinned[0]["sat"] is None
    assert pinned[1]["proof"] == [[]]


def test_solvers_dpll_refutation():
    for n in ("hand4", "hand5", "hand0", "ksat12", "mixed3", "deep"):
        f = FORMULA[n]
        sat, cert = solvers.dpll_refutation(f)
        assert sat == solvers.dpll_solve(f)[0] == (not _unsat(n))
        if sat:
            assert cert == solvers.dpll_solve(f)[1]
            assert n == "hand0" or solvers.check_assignment(f, cert)
        else:
            assert cert[-1] == [] and solvers.check_refutation(f, cert)
            core = solvers.trim_refutation(f, cert)
            assert core is not None and solvers.check_refutation(*core)
    both = solvers.dpll_refutation_batch([FORMULA["hand4"], FORMULA["hand5"]])
    assert both[0] == (False, [[-1], [1], []]) and both[1][0] is True


def test_logging_refuses_ref_mode_and_caller_assignments():
    for kw in (dict(mode="ref"), dict(inits=[[1]])):
        with pytest.raises(_capi.SatmiError, match=r"\(-1\)"):
            dpll_refutations([FORMULA["hand4"]], **kw)
