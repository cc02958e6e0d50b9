"""The Davis-Putnam kernels (csrc/dp.hip) outside the layout class of
test_dp_gpu.py: key widths K = 2 .. 10 and beyond, the model set and the
first-position table in LDS and in global memory, clause lists past the
split's small-run and packed-scan forms, key-width changes on one pooled
workspace, and the overflow-and-resume paths, counted.

Every comparison is exact against the oracle's recorded run
(tests/dp_paths.py; tests/test_dp_paths.py proves each row reaches what it is
named for): the verdict, the eliminated variables, and every clause list with
its clause order and each clause's set iteration order.  -1 only where the
step limit given to both sides produces it.  No time limits.  Each row runs
on the default pipeline and with SATMI_DP_INLINE=1, recorded (one step per
batch) and three times unrecorded (the batched path: enqueued, captured,
replayed)."""
import pytest

import dp_paths as P
from conftest import clause_list_sha
from satmi import _capi
from satmi.dp import eliminate, last_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["pipeline", "inline"])
def dp_mode(request, monkeypatch):
    if request.param == "inline":
        monkeypatch.setenv("SATMI_DP_INLINE", "1")
    else:
        monkeypatch.delenv("SATMI_DP_INLINE", raising=False)
    return request.param


def run_recorded(name):
    return eliminate(P.row_formula(name), step_limit=P.ROWS[name][1], record=True)


def assert_recorded(name, r, digest=False):
    o = P.row_oracle(name)
    assert r["result"] == o["result"], name
    assert r["vars"] == o["vars"], name
    assert len(r["clauses"]) == len(o["clauses"]), name
    for k, (got, want) in enumerate(zip(r["clauses"], o["clauses"])):
        if digest:   # long lists: by length and digest, both ends in full
            assert len(got) == len(want), (name, k)
            assert got[:50] == want[:50] and got[-50:] == want[-50:], (name, k)
            assert clause_list_sha(got) == clause_list_sha(want), (name, k)
        else:
            assert got == want, (name, k)


def assert_unrecorded(name, times=3):
    o = P.row_oracle(name)
    for _ in range(times):
        r = eliminate(P.row_formula(name), step_limit=P.ROWS[name][1])
        assert (r["result"], r["vars"]) == (o["result"], o["vars"]), name


def check_row(name, digest=False):
    assert_recorded(name, run_recorded(name), digest)
    assert_unrecorded(name)
    assert last_stats()["words"] == P.key_words(P.ROWS[name][2])


@pytest.mark.parametrize("name", P.KEY_WIDTH_ROWS)
def test_key_widths(name, dp_mode):
    """V on both sides of every 64-variable boundary up to 257: the K = 2, 4,
    6, 8 instances of the subset tests and the run-time-width one, the strided
    key loops, the split's word index, the inline tests at K <= 8 and the
    inline form's refusal at K = 10."""
    check_row(name)


@pytest.mark.parametrize("name", P.POPSET_ROWS)
def test_pop_set_placement(name, dp_mode):
    """The model set of variables.pop() in LDS (V = 255) and in global scratch
    (V = 256, 300), with ids that make the set be built."""
    check_row(name)


@pytest.mark.parametrize("name", P.FIRSTPOS_ROWS)
def test_first_position_placement(name, dp_mode):
    """V = 2048: the last size with the first-position table, the rank loop
    and the insertion order in LDS; V = 2049: all three in global memory, more
    than 64 key words per clause, and no inline step."""
    check_row(name)


@pytest.mark.parametrize("name", P.LARGE_ROWS)
def test_large_lists(name, dp_mode):
    """Lists past the split's 16-clause runs (packed scan), past 65,536
    clauses (three scans), 90,000 pairs in one step, and a neg list of 2^15
    clauses or more under the packed scan."""
    check_row(name, digest=True)


def test_key_width_changes_on_one_workspace(dp_mode):
    """One workspace through K = 2, 4, 10, 2, 6, 2: every K-sized buffer is
    laid out again, the hash table, the stamps and the pair capacity carry
    over.  Recorded, then unrecorded."""
    _capi.trim_workspaces()
    for name in P.WIDTH_CHANGE_SEQUENCE:
        assert_recorded(name, run_recorded(name))
    for name in P.WIDTH_CHANGE_SEQUENCE:
        assert_unrecorded(name, times=1)
    for name in P.WIDTH_CHANGE_SEQUENCE:
        assert_recorded(name, run_recorded(name))


@pytest.mark.parametrize("name", list(P.RESUME_ROWS))
def test_resumes(name, dp_mode):
    """On a fresh workspace the row outgrows the buffers dp_paths.forced_resumes
    derives from the oracle's record (all four between the rows): each is
    counted (satmi_dp_last_resumes), every list still equals the oracle's, and
    the same call again -- the workspace now large enough -- resumes nowhere."""
    _capi.trim_workspaces()
    r = run_recorded(name)
    first = last_stats()["resumes"]
    print(name, dp_mode, "resumes", first)
    assert_recorded(name, r, digest=name in P.LARGE_ROWS)
    for key in P.RESUME_ROWS[name]:
        assert first[key] >= 1, (name, key, first)
    r2 = run_recorded(name)
    assert last_stats()["resumes"] == dict.fromkeys(P.RESUME_KEYS, 0)
    assert (r2["result"], r2["vars"]) == (r["result"], r["vars"]) and r2["clauses"] == r["clauses"]
    # unrecorded, fresh again: the batched path resumes too
    _capi.trim_workspaces()
    assert_unrecorded(name, times=1)
    again = last_stats()["resumes"]
    for key in P.RESUME_ROWS[name]:
        assert again[key] >= 1, (name, key, again)
    assert_unrecorded(name, times=2)
    assert last_stats()["resumes"] == dict.fromkeys(P.RESUME_KEYS, 0)
