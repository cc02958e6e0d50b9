"""CPU checks of tests/res_paths.py: every row reaches the path of
csrc/resolution.hip it is named for -- by the model of the first packed pass
(tile height, wins per tile, claims per stripe, spill / key room on a fresh
workspace), by the pair kernel's flush and chunk arithmetic, and by the
oracle's record -- and every path has a row.  The constants come from the
.hip text: an edit there fails here instead of silently un-aiming a row."""
import json
import os

import pytest

import oracle
import res_paths as P
from conftest import clause_set_sha


def test_constants_read_from_the_source():
    C = P.hip_constants()
    assert (C["RES_TJ"], C["RES_ABUF"], C["RES_TILES"], C["RES_STRIPES"]) == (32, 1024, 16384, 64)
    assert (C["PAIR_BUF"], C["PAIR_CHUNK"], C["PAIR_WIDTHS"]) == (2048, 1 << 27, (0, 1, 2, 3, 4))


def test_every_path_has_a_row():
    for path, rows in P.PATHS.items():
        assert rows, path
        for name in rows:
            base = name.replace("limit_", "").replace("record_trunc_", "")
            f, _ = P.row(base)
            packed = len(P.variables(f)) <= 31
            assert packed == path.startswith("packed"), (path, name)
    # the issue's list of unrun paths, each owned by a key of PATHS
    for word in ("spill", "key room", "RES_ABUF", "batches", "max_passes", "clause_limit", "record truncation",
                 "WT =", "PAIR_BUF", "PAIR_CHUNK", "table rebuild", "clause growth"):
        assert any(word in path for path in P.PATHS), word
    assert sum("clause_limit" in p for p in P.PATHS) == sum("record truncation" in p for p in P.PATHS) == 2


@pytest.mark.parametrize("name", list(P.PRODUCT_ROWS))
def test_product_rows_against_model_and_oracle(name):
    """The construction {S_i u T_j} is what the model's first pass adds and
    what the oracle adds; the second pass adds nothing (True)."""
    f, want = P.row(name)
    m = P.model(name)
    assert m["new"] == want
    o = oracle.resolution(f, record=True)
    assert (o["result"], o["pass_new"]) == (1, [len(want)])
    assert [sorted(c) for c in o["clauses"][0]] == want


def test_stage_one_stripe():
    f, want = P.row("stage_one_stripe")
    m = P.model("stage_one_stripe")
    assert len(f) == 601 and len(P.variables(f)) == 11 and len(want) == 600
    assert (m["tj"], m["key_cap"], m["region"]) == (1, 16384, 512)
    assert m["tiles"] == {(600, 0): 256, (600, 1): 256, (600, 2): 88}     # one j, three i-tiles, one block x
    assert [s for s in m["stripes"] if s] == [600] and m["stripes"][600 % 64] == 600
    assert m["spill"] and not m["keys_over"] and not m["direct"]          # counter: stage 1, keys 0


def test_stage_present():
    f, want = P.row("stage_present")
    m = P.model("stage_present")
    assert len(f) == 641 and len(want) == 600 and m["tj"] == 1
    assert m["tiles"] == {(640, 0): 216, (640, 1): 256, (640, 2): 128}    # S_1 .. S_20 are input clauses: present
    assert m["stripes"][640 % 64] == 600 > m["region"] == 512
    assert m["spill"] and not m["keys_over"]


def test_keys_even():
    f, want = P.row("keys_even")
    m = P.model("keys_even")
    assert len(f) == 364 and len(P.variables(f)) == 16 and len(want) == 19200
    assert (m["tj"], m["key_cap"], m["region"]) == (1, 16384, 512)
    assert m["stripes"] == [300] * 64                                     # 64 consecutive j: every stripe once
    assert not m["spill"] and m["keys_over"] and not m["direct"]          # counter: keys 1, stage 0
    assert 364 + 19200 > 16384
    # the table of a fresh workspace (two slots per key of room) holds the pass at load <= 2/3: no table stop
    assert 2 * m["key_cap"] * 2 // 3 >= 364 + 19200


def test_abuf():
    f, want = P.row("abuf")
    m = P.model("abuf")
    C = P.hip_constants()
    assert len(f) == 6665 and len(P.variables(f)) == 27 and len(want) == 2560
    assert m["tj"] == 6665 * 14 // 16384 == 5 and 6655 == 5 * 1331
    assert m["tiles"] == {(1331, 0): 1280, (1332, 0): 1280}
    assert m["direct"] == {(1331, 0): 1280 - C["RES_ABUF"], (1332, 0): 1280 - C["RES_ABUF"]}
    assert (m["key_cap"], m["region"]) == (4 * 6665, 833)
    assert m["stripes"][1331 % 64] == m["stripes"][1332 % 64] == 1280 and sum(m["stripes"]) == 2560
    assert m["spill"] and not m["keys_over"]                              # the first run: stage 1, keys 0
    # the regrown region (5/4 of the fullest stripe + 1024) stores the direct appends of the rerun
    assert 1280 + 1280 // 4 + 1024 > 1280


def test_chain_rows():
    o = oracle.resolution(P.chain(30), record=True)
    assert (o["result"], o["pass_new"]) == (1, [29, 55, 98, 148, 105])    # 5 adding passes + the empty 6th: 2 batches of 4
    assert len(P.variables(P.chain(30))) == 30 and len(P.variables(P.chain(40))) == 40
    assert sum(o["pass_new"]) + 30 < 512                                  # no regrowth anywhere: the counter stays 0
    for n in (30, 40):
        full = oracle.resolution(P.chain(n))
        assert full["result"] == 1 and len(full["pass_new"]) >= 4
        cases = P.limit_cases(full["pass_new"], n)
        ps = [p for _, p in cases]
        assert ps[0] == 1 and ps[1] == 2 and ps[2] == ps[3] == 3 and ps[4] == 4 and ps[-1] is None
        assert ps[-2] == len(full["pass_new"])                            # the limit met by the last adding pass
        for lim, p in cases:   # the oracle's own clause_limit stops mid-pass: never more passes than p
            om = oracle.resolution(P.chain(n), clause_limit=lim)
            if p is not None:
                assert om["result"] == -1 and om["passes"] == p - 1, (n, lim)


@pytest.mark.parametrize("V", P.WIDTHS)
def test_width_rows(V):
    want_wt = dict(zip(P.WIDTHS, (1, 2, 2, 3, 3, 4, 4, 0, 0, 0)))
    f, _ = P.row("width_%d" % V)
    assert P.key_width(f) == (V, (V + 63) // 64, want_wt[V])
    o = oracle.resolution(f, max_passes=3, record=True)
    assert o["result"] == -1 and o["passes"] == 3
    assert sum(len(c) for p in o["clauses"] for c in p) < 1 << 20         # the record's capacity
    first = {tuple(sorted(c)) for c in o["clauses"][0]}
    Pk, Nk, dense = P.dense_keys(f)
    dec = P.decoder(f)
    assert all(dense[v] == v - 1 for v in dense)
    for d in P.named_dense(V):   # a pass-1 resolvent on dense variable d (bit 63, bit 0, the last word)
        hits = [(i, j, key) for i, j, key in _candidates_on(Pk, Nk, d)]
        assert hits, (V, d)
        assert any(tuple(dec(key)) in first for _, _, key in hits), (V, d)
    assert set(P.named_dense(V)) == {d for d in (63, 64, 127, 128) if d < V} | {V - 1}


def _candidates_on(Pk, Nk, d):
    bit = 1 << d
    pos = [i for i, p in enumerate(Pk) if p & bit]
    neg = [i for i, n in enumerate(Nk) if n & bit]
    for a in pos:
        for b in neg:
            i, j = min(a, b), max(a, b)
            c = (Pk[i] & Nk[j]) | (Nk[i] & Pk[j])
            rp, rn = (Pk[i] | Pk[j]) & ~c, (Nk[i] | Nk[j]) & ~c
            if c == bit and not rp & rn and rp | rn:
                yield i, j, (rp, rn)


@pytest.mark.parametrize("name,V,W,wt", [("pairbuf", 81, 2, 2), ("pairbuf_wide", 281, 5, 0)])
def test_pairbuf_rows(name, V, W, wt):
    f, want = P.row(name)
    assert P.key_width(f) == (V, W, wt) and len(want) == 2600
    fl = P.pair_flushes(f)
    assert fl == {len(f) - 1: [2048, 552]}                                # a mid-j flush of a full buffer, then the last
    if name == "pairbuf":
        o = oracle.resolution(f, record=True)
        assert (o["result"], o["pass_new"]) == (1, [2600])
        assert [sorted(c) for c in o["clauses"][0]] == want


def test_php43x3(golden_dir):
    f, _ = P.row("php43x3")
    assert len(f) == 66 and P.key_width(f) == (36, 1, 1)
    with open(os.path.join(golden_dir, "resolution_php43.json")) as fh:
        (c,) = json.load(fh)["cases"]
    counts = [p["count"] for p in c["passes"]]
    o = oracle.resolution(f, max_passes=3, record=True)
    assert o["pass_new"] == [3 * x for x in counts[:3]] == [108, 810, 21396]
    for k in range(3):   # every copy's clauses are the single formula's, renamed
        for part in P.php_project(o["clauses"][k]):
            assert clause_set_sha(part) == c["passes"][k]["sha256"]
    # pass 4: clauses [984, 22380), more pairs than one chunk
    jlo, ncl = 66 + 108 + 810, 66 + 108 + 810 + 21396
    ch = P.chunks(jlo, ncl)
    assert len(ch) == 2 and ch[0][0] == jlo and ch[-1][1] == ncl and ch[0][1] > 16384
    for k in range(3):
        assert len(P.chunks(*((0, 66), (66, 174), (174, 984))[k])) == 1
    # its 3 x 163,954 winners pass half of the table the pass starts with: a rebuild mid-pass
    assert ncl + 3 * counts[3] > P.table_slots(2 * ncl + 65536) // 2 > ncl
    # a fresh clause buffer grows in every pass
    assert P.clause_growths(66, 2, [108, 810, 21396, 3 * counts[3]]) == 4
