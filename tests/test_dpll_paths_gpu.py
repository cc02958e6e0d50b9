"""GPU: every row of tests/dpll_paths.py (the formulas test_dpll_paths.py proves
reach each structural path of csrc/dpll.hip) bit-exact against the oracle, in
the kernel's LDS form (KERNEL_GENERAL) and its wide form (KERNEL_WIDE), REF
and SOUND modes, batched into one launch and alone; the long-clause rows under
WIDE and AUTO, and TOO_LARGE under a pinned GENERAL; the LDS shape classes; a
wave's second instance."""
import pytest

import dpll_paths
from dpll_paths import CTR, DPLL_PATH_ROWS, LONG_ROWS, SHAPE_CLASS, SHAPE_ROWS
from satmi import _capi
from satmi.dpll import dpll_batch

pytestmark = pytest.mark.gpu

MODES = ("ref", "sound")
POLICY_NAMES = {_capi.KERNEL_AUTO: "auto", _capi.KERNEL_GENERAL: "general", _capi.KERNEL_WIDE: "wide"}
# rows that share a launch: everything but the shape rows (a batch shares its
# layout, so a shape row is its class only alone) and the long clauses
MAIN_ROWS = [r[0] for r in DPLL_PATH_ROWS if r[0] not in SHAPE_ROWS and r[0] not in LONG_ROWS]


def _kw(name):
    return dpll_paths.row(name)[2]


def _run(names, policy, mode):
    """One launch of the rows `names`, which share node_limit and sol_cap."""
    k = _kw(names[0])
    assert all((_kw(n)["node_limit"], _kw(n)["sol_cap"]) == (k["node_limit"], k["sol_cap"]) for n in names)
    _capi.set_kernel(policy)
    try:
        return dpll_batch([dpll_paths.row_formula(n) for n in names], mode=mode, max_solutions=0,
                          node_limit=k["node_limit"], sol_cap=k["sol_cap"],
                          inits=[_kw(n)["init"] or [] for n in names])
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)


def _dict_prefix(init):
    """The caller's dict as the trail's prefix: later values overwrite, the slot stays."""
    d = {}
    for x in init or []:
        d[abs(x)] = x
    return list(d.values())


def _mismatches(r, names, mode, tag):
    bad = []
    for b, name in enumerate(names):
        o = dpll_paths.row_oracle(name, mode)
        got = r.counter_dict(b)
        pre = _dict_prefix(_kw(name)["init"])
        checks = [("status", int(r.status[b]), o["status"])]
        checks += [(key, got[key], o["counters"][key]) for key in CTR]
        checks += [("solutions", r.solutions(b), o["solutions"]), ("root", r.root_assignment(b), o["root_assign"]),
                   ("dict prefix", r.root_assignment(b)[:len(pre)], pre),
                   ("root after the dict", r.root_assignment(b)[len(pre):], o["root_assign"][len(pre):])]
        for what, have, want in checks:
            if have != want:
                bad.append(f"{tag} {mode} {name}: {what} = {str(have)[:80]}, oracle {str(want)[:80]}")
    return bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", [_capi.KERNEL_GENERAL, _capi.KERNEL_WIDE], ids=["general", "wide"])
def test_rows_batched_match_oracle(policy, mode):
    """All rows but the shape and long-clause rows in one launch: the layout's caps
    are the batch's maxima (more than 4,096 clauses, 2,001 variables)."""
    shapes = [dpll_paths.shape_of(dpll_paths.row_formula(n), _kw(n)["init"] or ()) for n in MAIN_ROWS]
    caps = tuple(max(s[i] for s in shapes) for i in range(4))
    assert caps[1] > 4096 and caps[3] <= dpll_paths.NARROW_MAX_LEN
    _capi.set_kernel(policy)
    try:
        assert _capi.plan(*caps, mode=_capi.MODE_REF, has_init=True)[0] == policy
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    bad = _mismatches(_run(MAIN_ROWS, policy, mode), MAIN_ROWS, mode, POLICY_NAMES[policy])
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("name", MAIN_ROWS)
def test_row_alone_matches_oracle(name):
    """A row alone gets the tightest caps its sizes allow, in both forms and modes."""
    bad = []
    for policy in (_capi.KERNEL_GENERAL, _capi.KERNEL_WIDE):
        for mode in MODES:
            bad += _mismatches(_run([name], policy, mode), [name], mode, POLICY_NAMES[policy])
    assert not bad, bad[:8]


@pytest.mark.parametrize("name", list(SHAPE_ROWS))
def test_shape_row_matches_oracle_in_its_class(name):
    """The workgroup classes of the LDS form (4, 2, 1 waves; above 64 KiB of LDS
    per workgroup in the last two) and the 160 KiB bound, where AUTO and even a
    pinned GENERAL take the wide form."""
    shape = dpll_paths.shape_of(dpll_paths.row_formula(name))
    b, wpg = dpll_paths.lds_bytes(*shape[:3]), SHAPE_CLASS[name]
    bad = []
    for policy in (_capi.KERNEL_AUTO, _capi.KERNEL_GENERAL, _capi.KERNEL_WIDE):
        _capi.set_kernel(policy)
        try:
            kern, lds, waves = _capi.plan(*shape, mode=_capi.MODE_REF, has_init=True)
        finally:
            _capi.set_kernel(_capi.KERNEL_AUTO)
        if wpg == 0 or policy == _capi.KERNEL_WIDE:
            assert (kern, lds) == (_capi.KERNEL_WIDE, 256) and (wpg != 0 or b > dpll_paths.LDS_LIMIT)
        else:
            assert (kern, lds) == (_capi.KERNEL_GENERAL, b) and dpll_paths.narrow_shape(b) == (wpg, waves)
            assert (b * wpg > 64 * 1024) == (wpg < 4)
        if policy == _capi.KERNEL_AUTO:
            continue   # the same launch as GENERAL (or, past 160 KiB, as WIDE)
        for mode in MODES:
            bad += _mismatches(_run([name], policy, mode), [name], mode, POLICY_NAMES[policy])
    assert not bad, bad[:8]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", [_capi.KERNEL_WIDE, _capi.KERNEL_AUTO], ids=["wide", "auto"])
def test_long_clause_rows_match_oracle(policy, mode):
    """A clause of more than 255 literals in a batch whose sizes fit the LDS layout:
    AUTO plans and runs the wide form, beside the 255-literal row, batched and alone."""
    names = ["long_255"] + list(LONG_ROWS)
    shapes = [dpll_paths.shape_of(dpll_paths.row_formula(n)) for n in names]
    caps = tuple(max(s[i] for s in shapes) for i in range(4))
    assert 0 < dpll_paths.lds_bytes(*caps[:3]) <= dpll_paths.LDS_LIMIT and caps[3] == 300
    m = {"ref": _capi.MODE_REF, "sound": _capi.MODE_SOUND}[mode]
    _capi.set_kernel(policy)
    try:
        assert _capi.plan(*caps, mode=m, has_init=True)[0] == _capi.KERNEL_WIDE
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)
    bad = _mismatches(_run(names, policy, mode), names, mode, POLICY_NAMES[policy])
    for n in LONG_ROWS:
        bad += _mismatches(_run([n], policy, mode), [n], mode, POLICY_NAMES[policy] + " alone")
    assert not bad, bad[:8]


def test_long_clause_without_a_dict_takes_the_wide_form_under_auto():
    """The drop-in route: no caller's dict (SOUND mode is then open to the clause
    kernels, which a length above 5 rules out), one formula per call."""
    from satmi import solvers
    for name in LONG_ROWS:
        f = dpll_paths.row_formula(name)
        for mode in MODES:
            o = dpll_paths.row_oracle(name, mode)
            r = dpll_batch([f], mode=mode, max_solutions=0, node_limit=_kw(name)["node_limit"],
                           sol_cap=_kw(name)["sol_cap"])
            assert int(r.status[0]) == o["status"] and r.solutions(0) == o["solutions"], (name, mode)
            assert [r.counter_dict(0)[k] for k in CTR] == [o["counters"][k] for k in CTR], (name, mode)
    f = [list(range(1, 301)), [-1, -2]]
    import oracle
    want = oracle.dpll(f, "ref")
    assert want["status"] == 0 and want["solutions"]
    assert solvers.dpll_optimized(f) == [{abs(l): l > 0 for l in s} for s in want["solutions"]]
    sat, model = solvers.dpll_solve(f)
    assert sat and all(any(model.get(abs(l)) == (l > 0) for l in c) for c in f)


@pytest.mark.parametrize("mode", MODES)
def test_pinned_general_answers_too_large_per_instance(mode):
    """KERNEL_GENERAL pins the LDS form: the instances with a clause past 255
    literals get TOO_LARGE (zero counters, no root assignment), their neighbours
    the oracle's result; the drop-in solvers raise rather than read a verdict."""
    from satmi import solvers
    names = ["long_255", "long_300", "hub_101", "long_256", "emptied_129", "long_300_empty"]
    r = _run(names, _capi.KERNEL_GENERAL, mode)
    short = [n for n in names if n not in LONG_ROWS]
    for b, n in enumerate(names):
        if n in LONG_ROWS:
            assert int(r.status[b]) == _capi.DPLL_TOO_LARGE, n
            assert not r.counters[b, :7].any() and r.root_len[b] == 0 and r.solutions(b) == []
    bad = [m for m in _mismatches(r, names, mode, "general") if any(f" {n}:" in m for n in short)]
    assert not bad, bad[:8]
    _capi.set_kernel(_capi.KERNEL_GENERAL)
    try:
        with pytest.raises(_capi.SatmiError, match="too_large"):
            solvers.dpll_solve(dpll_paths.row_formula("long_300"))
        with pytest.raises(_capi.SatmiError, match="too_large"):
            solvers.dpll_optimized(dpll_paths.row_formula("long_300"))
    finally:
        _capi.set_kernel(_capi.KERNEL_AUTO)


@pytest.mark.parametrize("mode", MODES)
def test_second_tenant_sees_nothing_of_the_first(mode):
    """More instances than resident waves in the LDS form's one-wave class (one
    instance of 4,205 clauses sets the batch's layout): a wave's second instance
    re-stages its LDS slice after a conflict, a cut, a TOO_LARGE or a full
    search, and must equal the oracle as if it were the first."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kinds = ["long_300", "emptied_129", "units_200", "hub_101", "mismatch_149_sound", "fanout_decision_sound",
             "empty_first_64", "pures_398", "opposite_sign_same_chunk", "init_overwrite", "same_sign"]
    names = ["many_clauses"] + [kinds[b % len(kinds)] for b in range(cus + 64)]
    shapes = [dpll_paths.shape_of(dpll_paths.row_formula(n), _kw(n)["init"] or ()) for n in set(names)]
    lds = dpll_paths.lds_bytes(*(max(s[i] for s in shapes) for i in range(3)))
    assert dpll_paths.narrow_shape(lds) == (1, 1) and len(names) > cus   # one wave per CU: second tenants
    r = _run(names, _capi.KERNEL_GENERAL, mode)
    for b, n in enumerate(names):
        if n in LONG_ROWS:
            assert int(r.status[b]) == _capi.DPLL_TOO_LARGE, b
    bad = [m for m in _mismatches(r, names, mode, "general") if " long_300:" not in m]
    assert not bad, (len(bad), bad[:8])
