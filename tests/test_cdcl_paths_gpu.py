"""GPU: every row of tests/cdcl_paths.py (the formulas test_cdcl_paths.py proves
reach each structural path of csrc/cdcl.hip) bit-exact against the oracle, in
both placements of the per-variable arrays (LDS / arena); the placement
boundary; a wave's second instance; a full arena beside healthy neighbours;
a model row wider than the instance."""
import functools
import random

import pytest

import cdcl_paths
import oracle
from cdcl_paths import CDCL_PATH_ROWS, STAT_KEYS
from satmi import cnf
from satmi.cdcl import (CDCL_ERROR, CDCL_FULL, CDCL_LIMIT, CDCL_SAT, CDCL_UNSAT, CdclLimit, cdcl_batch,
                        cdcl_batch_packed)

pytestmark = pytest.mark.gpu

STATUS = {1: CDCL_SAT, 0: CDCL_UNSAT, -1: CDCL_LIMIT, -2: CDCL_ERROR}


def _check(r, o, tag=""):
    assert r["status"] == STATUS[o["result"]], tag
    assert r["assignment"] == o["assignment"], tag
    assert r["var_inc"] == o["var_inc"], tag   # bit for bit
    for k in STAT_KEYS:
        assert r["stats"][k] == o["stats"][k], (tag, k)


def lds_bytes(max_vars, max_len):
    """make_cdcl_layout's LDS image (csrc/cdcl.hip) restated: the per-variable
    and per-key arrays, each padded to 256 B, and two learned-literal lists of
    2 x (variables + 1) + 2 + the longest clause entries."""
    def a(x):
        return (x + 255) & ~255
    N = max_vars + 1
    K = 2 * N
    small = a(N) + a(8 * N) + a(4 * N) + a(4 * N) + a(8 * N) + a(8 * (N // 64 + 1)) + 6 * a(4 * K)
    return small + 4 * 2 * (2 * N + 2 + max(max_len, 1))


CDCL_LDS_MAX = 32768


def in_lds(formulas):
    nv = max(abs(l) for f in formulas for c in f for l in c)
    return lds_bytes(nv, max(len(c) for f in formulas for c in f)) <= CDCL_LDS_MAX


def random_3cnf(n, seed):
    """2n random 3-literal clauses over exactly n variables (n itself occurs)."""
    rng = random.Random(seed)
    f = [[v if rng.random() < 0.5 else -v for v in rng.sample(range(1, n + 1), 3)] for _ in range(2 * n)]
    f[0][0] = n
    return f


FILLER_VARS = 420   # beyond the LDS image with any clause length (test_cdcl_arena_form_beyond_lds)


@functools.lru_cache(maxsize=None)
def filler():
    return random_3cnf(FILLER_VARS, 77)


@functools.lru_cache(maxsize=None)
def filler_oracle(cap):
    return oracle.cdcl(filler(), cap)


@pytest.mark.parametrize("row", CDCL_PATH_ROWS, ids=[r[0] for r in CDCL_PATH_ROWS])
def test_row_matches_oracle_in_lds_and_arena(row):
    """Alone a row's launch keeps the small arrays in LDS; beside a formula of
    420 variables the launch takes the arena form for both."""
    name, _, cap, _ = row
    f, o = cdcl_paths.row_formula(name), cdcl_paths.row_oracle(name)
    assert in_lds([f]), "every row is small enough for the LDS form"
    _check(cdcl_batch([f], max_iter=cap)[0], o, f"{name} lds")
    assert not in_lds([f, filler()])
    r = cdcl_batch([f, filler()], max_iter=cap)
    _check(r[0], o, f"{name} arena")
    _check(r[1], filler_oracle(cap), f"{name} arena: filler")


def test_placement_boundary():
    """The largest variable count whose launch stays in LDS and the smallest that
    leaves it, for 3-literal clauses."""
    n = max(v for v in range(1, 1000) if lds_bytes(v, 3) <= CDCL_LDS_MAX)
    assert 300 < n < FILLER_VARS and lds_bytes(n + 1, 3) > CDCL_LDS_MAX
    for nv in (n, n + 1):
        f = random_3cnf(nv, 1000 + nv)
        assert in_lds([f]) == (nv == n)
        _check(cdcl_batch([f], max_iter=400)[0], oracle.cdcl(f, 400), f"n = {nv}")


SMALL = (
    [[1, 2], [-1, 2], [-2, 3]],            # SAT after three decisions
    [[1], [-1, -1]],                       # UNSAT at level 0
    [[-1, -2]],                            # loops (the reference's timeout rows)
    [[1, 2, 3]],
    [[2], [-2, 1], [-1, -2, 3, 4], [5, 6]],
    [[-1, -2, -3], [4, -5], [-6, 1]],
    [[-1, -1, -2, -2]],
)


def _large():
    """60-130 variables each: rows of the table, and both activity-bump forms
    with repeated variables (62 and 120 entries) so that they meet in one launch."""
    rows = [cdcl_paths.row_formula(n) for n in ("neg_130", "windows", "overlap", "neg_70", "neg_65")]
    return rows + [cdcl_paths.binary(60), cdcl_paths.doubled(60), cdcl_paths.doubled(2, 58)]


def test_second_tenant_sees_nothing_of_the_first():
    """More than twice as many instances as resident waves, a large formula
    (60-130 variables: many keys, grown tables, learned clauses, every appears
    word) then a tiny one, in turn: a wave's second instance reuses its arena
    and LDS image, and must equal the oracle as if it were the first."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus * 32 + 37
    cap = 200
    large = _large()
    assert all(60 <= max(abs(l) for c in f for l in c) <= 130 for f in large)
    kinds = large + [list(f) for f in SMALL]
    order = [(b // 2) % len(large) if b % 2 == 0 else len(large) + (b // 2) % len(SMALL) for b in range(B)]
    want = [oracle.cdcl(f, cap) for f in kinds]   # once per distinct formula
    rs = cdcl_batch([kinds[k] for k in order], max_iter=cap)
    assert len(rs) == B
    bad = []
    for b, (k, r) in enumerate(zip(order, rs)):
        try:
            _check(r, want[k], f"instance {b} kind {k}")
        except AssertionError as e:
            bad.append(str(e)[:200])
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("learn_cap", [1, 2, 50])
def test_full_arena_is_a_status_and_spares_the_neighbours(learn_cap):
    long = cdcl_paths.row_formula("neg_70")
    quiet = [[[1, 2]], [[1, 2], [-1, 2], [-2, 3]], [[1], [-1, -1]]]   # never learn
    cap = 5000
    rs = cdcl_batch([quiet[0], long, quiet[1], quiet[2]], max_iter=cap, learn_cap=learn_cap)
    assert rs[1]["status"] == CDCL_FULL
    assert 0 < rs[1]["stats"]["learned"] <= learn_cap
    for r, f in zip((rs[0], rs[2], rs[3]), quiet):
        o = oracle.cdcl(f, cap)
        assert o["stats"]["learned"] == 0
        _check(r, o, f"neighbour {f}")


def test_full_arena_raises_from_cdcl_solve():
    from satmi.cdcl import cdcl_solve
    with pytest.raises(CdclLimit, match="arena full"):
        cdcl_solve(cdcl_paths.row_formula("neg_70"), learn_cap=2)


def test_model_row_wider_than_the_instance():
    """assign_stride is the batch's largest variable count: an instance of 70
    variables beside one of 420 fills the first assign_len entries of its row."""
    f, cap = cdcl_paths.row_formula("neg_70"), 300
    out = cdcl_batch_packed(cnf.pack([f, filler()]), max_iter=cap, arrays=True)
    assert out["assign"].shape == (2, FILLER_VARS)
    for b, o in enumerate((cdcl_paths.row_oracle("neg_70"), filler_oracle(cap))):
        n = int(out["assign_len"][b])
        assert n == len(o["assignment"])
        assert out["assign"][b, :n].tolist() == o["assignment"]
        assert out["status"][b] == STATUS[o["result"]] and out["var_inc"][b] == o["var_inc"]
