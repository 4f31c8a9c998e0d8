"""GPU suite (-m gpu): the multiple sequence alignment and coverage of POA groups (vc_poa_run_msa, poa.poa_msa, the command
line's -r 1 / -r 2) byte for byte against spoa -- every entry of tests/golden/poa_msa.json.gz --, freshly seeded groups against
the CPU restatement tests/poa_msa_ref.py live with spoa's own invariants on every row, the host schedule under small budgets, the
degenerate groups, the flag-less call, the command line, and the other entry points unchanged beside it.  Each test prints its
time."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import poa_msa_ref as M
from poa_common import _done, _kw, _workers
from test_poa import load_fixture, members
from test_poa_msa import entries
from vechat_amd import capi, large, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_poa  # noqa: E402


def _same(a, b, label):
    assert a.rows == b.rows and a.members == b.members and a.consensus == b.consensus, label
    assert (a.coverage is None) == (b.coverage is None) and (a.coverage is None or a.coverage.tolist() == b.coverage.tolist()), label


# ------------------------------------------------------------------ 1. every fixture entry
def test_every_fixture_entry(built):
    t0 = time.time()
    calls = {}
    for label, mem, t, scores, e in entries():
        calls.setdefault((t, scores), []).append((label, mem, e))
    n = 0
    for (t, scores), es in calls.items():
        groups = [mem for _, mem, _ in es]
        got = poa.poa_msa(groups, t, include_consensus=True, coverage=True, **_kw(scores))
        cons = poa.poa_consensus(groups, t, **_kw(scores))
        plain = poa.poa_msa(groups, t, **_kw(scores))
        for (label, mem, e), m, c, p in zip(es, got, cons, plain):
            assert m.rows == [r.encode() for r in e["rows"]], label
            assert m.members == e["members"] + [poa.CONSENSUS_ROW], label
            assert m.consensus.decode() == e["consensus"] and m.consensus == c, label
            assert m.rows[-1].replace(b"-", b"") == m.consensus, label
            assert m.coverage.dtype == np.uint32 and m.coverage.tolist() == e["coverage"], label
            assert p.rows == m.rows[:-1] and p.members == e["members"] and p.coverage is None and p.consensus == c, label
            n += 1
    print(f"[fixture] {n} entries in {len(calls)} x 3 calls, rows, members, consensus and coverage byte-identical, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. fresh groups against the restatement, live
def _fresh(seed, n):
    rng = random.Random(seed)
    R = lambda k: bytes(rng.choice(b"ACGT") for _ in range(k))
    out = []
    for i in range(n):
        size = rng.choice([1, 2, 3, 4, 6, 8, 12, 20, 33, 64] if i % 8 else [1, 2, 3, 5])
        L = rng.choice([1, 5, 30, 80, 150, 300] if size > 20 else [1, 5, 30, 80, 150, 300, 505, 520, 600])
        g = make_poa.members_of(rng, R(L), size, rate=rng.choice([0.02, 0.08, 0.15]), fastq=rng.random(), rc=rng.choice([0, 0, 0.3]),
                                partial=rng.choice([0, 0.4]))
        if i % 5 == 0:                                                     # empty members at the front / middle / end
            for at in {0: [0], 1: [len(g) // 2], 2: [len(g)], 3: [0, len(g) // 2, len(g) + 2]}[(i // 5) % 4]:
                g.insert(min(at, len(g)), (b"", None))
        if i % 7 == 0:                                                     # IUPAC bytes
            s = bytearray(g[-1][0])
            for k in range(0, len(s), 3):
                s[k] = rng.choice(b"NRYSWKMBDHV")
            g[-1] = (bytes(s), g[-1][1])
        out.append(g)
    return out


def _ref_job(a):
    g, t = a
    return M.msa(g, t, 5, -4, -8, include_consensus=True)


@pytest.mark.parametrize("t", [0, 1, 2])
def test_fresh_groups_against_the_restatement(built, t):
    groups = _fresh(9100 + t, 300)
    t0 = time.time()
    got = poa.poa_msa(groups, t, include_consensus=True, coverage=True)
    t1 = time.time()
    rows = 0
    for g, m in zip(groups, got):                                          # independent of any restatement: every row of every group
        M.check_invariants(m.rows, m.members, g, True)
        assert m.rows[-1].replace(b"-", b"") == m.consensus and len(m.coverage) == len(m.consensus)
        rows += len(m.rows)
    with ProcessPoolExecutor(_workers()) as ex:
        ref = list(ex.map(_ref_job, [(g, t) for g in groups], chunksize=4))
    for w, (m, r) in enumerate(zip(got, ref)):
        assert m.rows == r["rows"] and m.members == r["members"] and m.consensus == r["consensus"], (t, w)
        assert m.coverage.tolist() == r["coverage"], (t, w)
    print(f"[fresh groups, algorithm {t}] {len(groups)} groups, {rows} rows equal the restatement and hold spoa's invariants; "
          f"device {t1 - t0:.1f} s, restatement {time.time() - t1:.1f} s")


# ------------------------------------------------------------------ 3. the host schedule under small budgets
def test_msa_under_small_budgets(built, monkeypatch, capfd):
    fx = load_fixture()
    fixed = [g for g in fx["groups"] if tuple(g["scores"]) == (5, -4, -8) and len(g["seqs"]) <= 17]
    fresh = _fresh(9200, 1024)
    groups = fresh[:500] + [members(g) for g in fixed] + fresh[500:]
    want = poa.poa_msa(groups, "semi-global", include_consensus=True, coverage=True)
    env = (("VC_LARGE_CAPS", "l:3"), ("VC_LARGE_ARENA_MB", "24"), ("VC_LARGE_MAT_MB", "0.5"), ("VC_LARGE_LOG", "1"))
    for k, v in env:
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    t0 = time.time()
    try:
        got = poa.poa_msa(groups, "semi-global", include_consensus=True, coverage=True)
    finally:
        for k, _ in env:
            monkeypatch.delenv(k)
    dt = time.time() - t0
    err = capfd.readouterr().err
    ev = [l[len("vc_large: "):].split()[0] for l in err.splitlines() if l.startswith("vc_large: ")]
    regrown = [l for l in err.splitlines() if l.startswith("vc_large: regrow") and "labels" in l]
    msa_line = re.search(r"vc_large: msa launches=(\d+) bytes=(\d+)", err)
    assert regrown and ev.count("group") >= 3 and ev.count("step") >= 1 and msa_line, {e: ev.count(e) for e in set(ev)}
    assert int(msa_line.group(1)) >= 3 and int(msa_line.group(2)) > 0      # (a batch whose groups all regrow launches none)
    for w, (a, b) in enumerate(zip(got, want)):
        _same(a, b, w)
    es = {l: e for l, _, _, _, e in entries()}
    for k, g in enumerate(fixed):
        assert got[500 + k].rows == [r.encode() for r in es[g["name"] + "/2"]["rows"]], g["name"]
    print(f"[small budgets] {len(groups)} groups in {dt:.1f} s; events {({e: ev.count(e) for e in set(ev)})}; "
          f"{len(regrown)} label regrowths; msa launches {msa_line.group(1)}, bytes {msa_line.group(2)}")


# ------------------------------------------------------------------ 4. degenerate groups beside valid ones
def test_degenerate_groups_beside_valid_ones(built, monkeypatch):
    """An empty group and a group of empty sequences: VC_WIN_OK, no row and row_size 0 (with the consensus row: that row alone,
    of length 0).  No input of testable size makes the reference throw on a POA group (every fixture entry is VC_WIN_OK; the score
    floor needs graphs of millions of nodes at int8 scores), so the not-computed case is a group the arena budget refuses,
    VC_WIN_OVERFLOW: zero rows through the same test in the host schedule (status != VC_WIN_OK), neighbours unaffected."""
    t0 = time.time()
    valid = _fresh(9300, 6)
    big = make_poa.members_of(random.Random(5), bytes(random.Random(6).choice(b"ACGT") for _ in range(3000)), 24)
    groups = [valid[0], [], valid[1], [(b"", None), (b"", None)], valid[2], big, valid[3]]
    alone = [poa.poa_msa([g], include_consensus=True, coverage=True)[0] for g in groups]
    for cons_row in (False, True):
        got = poa.poa_msa(groups, include_consensus=cons_row, coverage=True)
        for w in (1, 3):
            assert got[w].rows == ([b""] if cons_row else []) and got[w].members == ([poa.CONSENSUS_ROW] if cons_row else [])
            assert got[w].consensus == b"" and got[w].coverage.size == 0
        for w in (0, 2, 4, 5, 6):
            assert got[w].rows == (alone[w].rows if cons_row else alone[w].rows[:-1]) and got[w].coverage.tolist() == alone[w].coverage.tolist()
    monkeypatch.setenv("VC_LARGE_ARENA_MB", "4")
    try:
        with pytest.raises(poa.PoaError) as ex:
            poa.poa_msa(groups, include_consensus=True, coverage=True)
        assert ex.value.groups == {5: capi.VC_WIN_OVERFLOW}
        got = poa.poa_msa(groups, include_consensus=True, coverage=True, strict=False)
        res, status = poa.run_batch_msa(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, 5, -4, -8, -8, -8, -8), 7)
    finally:
        monkeypatch.delenv("VC_LARGE_ARENA_MB")
    assert got[5] is None and int(status[5]) == capi.VC_WIN_OVERFLOW
    assert res[5].rows == [] and res[5].members == [] and res[5].consensus == b"" and res[5].coverage.size == 0
    for w in (0, 1, 2, 3, 4, 6):
        _same(got[w], alone[w], w)
    print(f"[degenerate groups] empty, empty-sequences and refused groups beside valid ones, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. without flags: vc_poa_run_gaps
def test_without_flags_it_is_vc_poa_run_gaps(built, monkeypatch, capfd):
    groups = _fresh(9400, 64)
    batch = poa.group_batch(groups)
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    try:
        for p in (capi.VcPoaGapParams(0, 1, 5, -4, -8, -8, -8, -8), capi.VcPoaGapParams(0, 2, 5, -4, -8, -6, -10, -4)):
            capfd.readouterr()
            res, st0 = poa.run_batch_msa(batch, p, 0)
            e0 = capfd.readouterr().err
            cons, st1 = poa.run_batch(batch, p)
            e1 = capfd.readouterr().err
            res7, st7 = poa.run_batch_msa(batch, p, 7)
            e7 = capfd.readouterr().err
            assert [m.consensus for m in res] == cons == [m.consensus for m in res7] and st0.tolist() == st1.tolist() == st7.tolist()
            assert all(m.rows == [] and m.members == [] and m.coverage is None for m in res)
            assert _done(e0) == _done(e1) == _done(e7) and len(_done(e0)) == 1      # the same alignments and cells
            assert "vc_large: msa" not in e0 and "vc_large: msa" in e7
    finally:
        monkeypatch.delenv("VC_LARGE_LOG")
    # the library's arrays are NULL without flags
    lib = capi.load_hip()
    o = capi.VcPoaMsaOut(flags=0)
    cons = np.zeros(int(batch.bases.size), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(batch.n_windows, np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    assert lib.vc_poa_run_msa(C.byref(capi.VcPoaGapParams(0, 1, 5, -4, -8, -8, -8, -8)), C.byref(vb), C.byref(r), C.byref(o)) == 0
    assert o.n_groups == batch.n_windows and not o.n_rows and not o.rows and not o.coverage and o.rows_bytes == 0


# ------------------------------------------------------------------ 6. the command line
def test_command_line_msa_on_the_sample(built):
    sample = os.path.join(GOLDEN, "sample.fastq.gz")
    names = [l[1:].split()[0] for l in __import__("gzip").open(sample, "rt").read().split("\n")[0::4] if l]
    es = {l: e for l, _, _, _, e in entries()}
    t0 = time.time()
    for lvl, key in (("0", "LocalWithQualities"), ("1", "GlobalWithQualities"), ("2", "SemiGlobalWithQualities")):
        rows = es[key]["rows"]
        for r, keep in (("1", rows[:-1]), ("2", rows)):
            p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", lvl, "-r", r, sample], cwd=ROOT, capture_output=True, timeout=300)
            assert p.returncode == 0, p.stderr.decode()
            want = "".join(f">{n}\n{row}\n" for n, row in zip(names + ["Consensus"], keep))
            assert p.stdout.decode() == want, (lvl, r)
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--coverage", sample], cwd=ROOT, capture_output=True, timeout=300)
    e = es["GlobalWithQualities"]
    assert p.returncode == 0 and p.stdout.decode() == (f">Consensus LN:i:{len(e['consensus'])} CV:B:I," + ",".join(map(str, e["coverage"]))
                                                       + f"\n{e['consensus']}\n")
    print(f"[command line] -r 1 / -r 2 x -l 0 / 1 / 2 and --coverage on the sample, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 7. the other entry points before and after, sharing the buffer cache
def test_other_paths_unchanged_beside_the_msa(built):
    gold = fixtures.load_windows()
    batch = fixtures.fixture_batch(gold["windows"])
    fx = load_fixture()
    g = next(g for g in fx["groups"] if g["name"] == "size64_len300_partial")

    def check(label):
        for mode, key in ((0, "hap"), (1, "linear")):
            cons, status = large.large_consensus(batch, capi.default_params(mode=mode))
            for w, win in enumerate(gold["windows"]):
                exp = win["expected"][key]
                assert cons[w].decode() == exp["consensus"], (label, mode, win["name"])
                assert (int(status[w]) == capi.VC_WIN_OK) == exp["polished"], (label, mode, win["name"])
        assert poa.poa_consensus([members(g)], "global")[0].decode() == g["expected"]["1"]["consensus"], label
    t0 = time.time()
    check("before")
    e = {l: x for l, _, _, _, x in entries()}["size64_len300_partial/1"]
    m = poa.poa_msa([members(g)], "global", include_consensus=True, coverage=True)[0]
    assert m.rows == [r.encode() for r in e["rows"]] and m.coverage.tolist() == e["coverage"]
    check("after")
    large.release()
    m = poa.poa_msa([members(g)], "global", include_consensus=True)[0]
    assert m.rows == [r.encode() for r in e["rows"]]
    check("after a release")
    print(f"[other paths beside the MSA] {len(gold['windows'])} golden windows x 2 modes and vc_poa_run, three times, {time.time() - t0:.1f} s")
