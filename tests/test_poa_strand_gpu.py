"""GPU suite (-m gpu): strand-ambiguous POA groups (vc_poa_run_strand, poa.poa_consensus_strands, poa.poa_msa(strand_ambiguous=
True), the command line's --both-strands) byte for byte against spoa's `-s` -- every entry of tests/golden/poa_strand.json.gz --,
freshly seeded groups with random flips against the CPU restatement tests/poa_strand_ref.py and against the already pinned
vc_poa_run_msa on the kept views, the host schedule under small budgets, degenerate and refused groups, the plain calls unchanged
beside it, and the command line.  Each test prints its time."""
import gzip
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
import poa_strand_ref as S
from poa_common import MODELS, _done, _kw, _workers
from test_poa import load_fixture, members
from test_poa_strand import entries, flipped
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_poa  # noqa: E402



def _params(t, scores):
    return capi.VcPoaGapParams(0, t, *scores)


def _strand(groups, t, scores, flags=7):
    """-> (list of Msa with .reversed, status, forward scores, reverse scores)"""
    return poa.run_batch_msa(poa.group_batch(groups), _params(t, scores), flags, strands=True)


def _kept(g, rev):
    return [S.kept_view(s, q, bool(r)) for (s, q), r in zip(g, rev)]


# ------------------------------------------------------------------ 1. every fixture entry
def test_every_fixture_entry(built):
    t0 = time.time()
    calls = {}
    for label, mem, t, scores, e in entries():
        calls.setdefault((t, scores), []).append((label, mem, e))
    n = 0
    for (t, scores), es in calls.items():
        groups = [mem for _, mem, _ in es]
        got, status, sc, scr = _strand(groups, t, scores)
        cons, rev = poa.poa_consensus_strands(groups, t, **_kw(scores))
        assert status.tolist() == [capi.VC_WIN_OK] * len(groups)
        for (label, mem, e), m, a, b, c, r in zip(es, got, sc, scr, cons, rev):
            assert m.reversed.tolist() == [bool(x) for x in e["reversed"]] == r.tolist(), label
            assert a.tolist() == e["score"] and b.tolist() == e["score_rev"], label
            assert m.rows == [x.encode() for x in e["rows"]], label
            assert m.members == e["members"] + [poa.CONSENSUS_ROW], label
            assert m.consensus.decode() == e["consensus"] and m.consensus == c, label
            assert m.coverage.dtype == np.uint32 and m.coverage.tolist() == e["coverage"], label
            n += 1
    print(f"[fixture] {n} entries in {len(calls)} x 2 calls: flags, both scores, rows, members, consensus and coverage "
          f"byte-identical, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. fresh groups: the restatement, and the pinned path on the kept views
def _fresh(seed, n):
    """seeded groups of noisy copies, members flipped at random (member 0 too), some empty members, some IUPAC bytes"""
    rng = random.Random(seed)
    R = lambda k: bytes(rng.choice(b"ACGT") for _ in range(k))            # noqa: E731
    out = []
    for i in range(n):
        size = rng.choice([1, 2, 3, 4, 6, 8, 12, 20, 33] if i % 8 else [1, 2, 3, 5])
        L = rng.choice([1, 5, 30, 80, 150, 300] if size > 12 else [1, 5, 30, 80, 150, 300, 505, 520, 600])
        g = make_poa.members_of(rng, R(L), size, rate=rng.choice([0.02, 0.08, 0.15]), fastq=rng.random(), partial=rng.choice([0, 0.4]))
        if i % 5 == 0:
            for at in {0: [0], 1: [len(g) // 2], 2: [len(g)], 3: [0, len(g) // 2, len(g) + 2]}[(i // 5) % 4]:
                g.insert(min(at, len(g)), (b"", None))
        if i % 7 == 0:
            s = bytearray(g[-1][0])
            for k in range(0, len(s), 3):
                s[k] = rng.choice(b"NRYSWKMBDHV")
            g[-1] = (bytes(s), g[-1][1])
        out.append(flipped(g, [k for k in range(len(g)) if rng.random() < 0.5]))
    return out


def _ref_job(a):
    g, t, scores = a
    return S.strands(g, t, *scores, include_consensus=True)


@pytest.mark.parametrize("t", [0, 1, 2])
def test_fresh_groups_against_the_restatement_and_the_plain_path(built, t):
    groups = _fresh(9500 + t, 300)
    t0 = time.time()
    got, n_rev = [None] * len(groups), 0
    model_of = [list(MODELS)[w % 3] for w in range(len(groups))]
    for model, scores in MODELS.items():
        idx = [w for w in range(len(groups)) if model_of[w] == model]
        sub = [groups[w] for w in idx]
        res, status, sc, scr = _strand(sub, t, scores)
        assert status.tolist() == [capi.VC_WIN_OK] * len(sub)
        # the normalisation identity: the kept views through the pinned vc_poa_run_msa give the same bytes, and the strand call
        # on them keeps every member forward and reports the same consensus
        norm = [_kept(g, m.reversed) for g, m in zip(sub, res)]
        plain = poa.poa_msa(norm, t, include_consensus=True, coverage=True, **_kw(scores))
        again, again_rev = poa.poa_consensus_strands(norm, t, **_kw(scores))
        for w, m, p, c, r, a, b in zip(idx, res, plain, again, again_rev, sc, scr):
            assert (m.rows, m.members, m.consensus, m.coverage.tolist()) == (p.rows, p.members, p.consensus, p.coverage.tolist()), (t, w)
            assert c == m.consensus and not r.any(), (t, w)
            got[w] = (m, a, b)
            n_rev += int(m.reversed.sum())
    t1 = time.time()
    with ProcessPoolExecutor(_workers()) as ex:
        ref = list(ex.map(_ref_job, [(g, t, MODELS[model_of[w]]) for w, g in enumerate(groups)], chunksize=4))
    for w, ((m, a, b), r) in enumerate(zip(got, ref)):
        assert m.reversed.tolist() == r["reversed"] and a.tolist() == r["score"] and b.tolist() == r["score_rev"], (t, w)
        assert m.rows == r["rows"] and m.members == r["members"] and m.consensus == r["consensus"], (t, w)
        assert m.coverage.tolist() == r["coverage"], (t, w)
    assert n_rev > 300
    print(f"[fresh groups, algorithm {t}] {len(groups)} groups over linear / affine / convex gaps, {n_rev} members kept reversed: equal "
          f"to the restatement and to vc_poa_run_msa on the kept views; device {t1 - t0:.1f} s, restatement {time.time() - t1:.1f} s")


# ------------------------------------------------------------------ 3. the host schedule under small budgets
def test_strands_under_small_budgets(built, monkeypatch, capfd):
    fx = load_fixture()
    fixed = [flipped(members(g), range(1, len(g["seqs"]), 2)) for g in fx["groups"]
             if tuple(g["scores"]) == (5, -4, -8) and len(g["seqs"]) <= 17]
    fresh = _fresh(9600, 384)
    groups = fresh[:200] + fixed + fresh[200:]
    scores = MODELS["affine"]
    want, st, wsc, wscr = _strand(groups, 2, scores)
    assert st.tolist() == [capi.VC_WIN_OK] * len(groups)
    norm = [_kept(g, m.reversed) for g, m in zip(groups, want)]
    env = (("VC_LARGE_CAPS", "n:5,e:5,a:7,l:3,s:10,p:6"), ("VC_LARGE_ARENA_MB", "24"), ("VC_LARGE_MAT_MB", "0.5"), ("VC_LARGE_LOG", "1"))
    for k, v in env:
        monkeypatch.setenv(k, v)
    t0 = time.time()
    try:
        capfd.readouterr()
        got, st, sc, scr = _strand(groups, 2, scores)
        err = capfd.readouterr().err
        plain = poa.poa_msa(norm, 2, include_consensus=True, coverage=True, **_kw(scores))
        err_plain = capfd.readouterr().err
    finally:
        for k, _ in env:
            monkeypatch.delenv(k)
    dt = time.time() - t0
    lines = [l for l in err.splitlines() if l.startswith("vc_large: ")]
    ev = [l[len("vc_large: "):].split()[0] for l in lines]
    grown = set()
    for l in lines:
        if l.startswith("vc_large: regrow"):
            grown |= set(re.search(r"flags=(\S+)", l).group(1).split(","))
    steps = [tuple(map(int, re.match(r"vc_large: step launches=(\d+) over=(\d+)", l).groups())) for l in lines if l.startswith("vc_large: step")]
    assert grown == {"nodes", "edges", "aligned", "labels", "stack", "pairs"}, grown      # every table regrew in strand mode
    assert ev.count("group") >= 2 and steps and max(k for k, _ in steps) >= 3              # steps split into several forward launches
    assert any(o >= 1 for _, o in steps)                                                   # a pair above the budget ran alone
    assert st.tolist() == [capi.VC_WIN_OK] * len(groups)
    for w, (a, b, p) in enumerate(zip(got, want, plain)):
        assert (a.rows, a.members, a.consensus, a.coverage.tolist()) == (b.rows, b.members, b.consensus, b.coverage.tolist()), w
        assert a.reversed.tolist() == b.reversed.tolist() and sc[w].tolist() == wsc[w].tolist() and scr[w].tolist() == wscr[w].tolist(), w
        assert (a.rows, a.consensus, a.coverage.tolist()) == (p.rows, p.consensus, p.coverage.tolist()), w
    (al, cells), (al_plain, cells_plain) = _done(err)[0], _done(err_plain)[0]
    assert len(_done(err)) == 1 and al == 2 * al_plain and cells == 2 * cells_plain and al_plain > 0, (al, al_plain, cells, cells_plain)
    print(f"[small budgets] {len(groups)} groups in {dt:.1f} s; events {({e: ev.count(e) for e in set(ev)})}; regrown {sorted(grown)}; "
          f"alignments {al} = 2 x {al_plain}; most launches in a step {max(k for k, _ in steps)}, "
          f"{sum(1 for _, o in steps if o)} steps with a pair above the budget")


# ------------------------------------------------------------------ 4. degenerate and refused groups beside valid ones
def test_degenerate_and_refused_groups_beside_valid_ones(built, monkeypatch):
    """No input of testable size makes the reference throw on a POA group, so the not-computed group is one the arena budget
    refuses (VC_WIN_OVERFLOW), as in tests/test_poa_msa_gpu.py: zeros in the strand output, the neighbours computed."""
    t0 = time.time()
    valid = _fresh(9700, 6)
    big = flipped(make_poa.members_of(random.Random(5), bytes(random.Random(6).choice(b"ACGT") for _ in range(3000)), 24), range(1, 24, 2))
    groups = [valid[0], [], valid[1], [(b"", None), (b"", None)], valid[2], big, valid[3]]
    sc6 = MODELS["linear"]
    alone = [_strand([g], 1, sc6) for g in groups]
    got, status, sc, scr = _strand(groups, 1, sc6)
    assert status.tolist() == [capi.VC_WIN_OK] * 7
    assert got[1].reversed.size == 0 and got[3].reversed.tolist() == [False, False] and sc[3].tolist() == [0, 0] == scr[3].tolist()
    assert got[1].rows == [b""] and got[3].rows == [b""] and got[1].consensus == b"" == got[3].consensus
    assert got[5].reversed.tolist() == [bool(k & 1) for k in range(24)]
    for w in range(7):
        assert (got[w].rows, got[w].consensus, got[w].reversed.tolist(), sc[w].tolist(), scr[w].tolist()) == \
               (alone[w][0][0].rows, alone[w][0][0].consensus, alone[w][0][0].reversed.tolist(), alone[w][2][0].tolist(), alone[w][3][0].tolist()), w
    monkeypatch.setenv("VC_LARGE_ARENA_MB", "4")
    try:
        with pytest.raises(poa.PoaError) as ex:
            poa.poa_consensus_strands(groups)
        assert ex.value.groups == {5: capi.VC_WIN_OVERFLOW}
        cons, rev, s0, s1 = poa.poa_consensus_strands(groups, strict=False, scores=True)
        res, status, sc2, scr2 = _strand(groups, 1, sc6)
    finally:
        monkeypatch.delenv("VC_LARGE_ARENA_MB")
    assert cons[5] is None and int(status[5]) == capi.VC_WIN_OVERFLOW and res[5].rows == [] and res[5].consensus == b""
    for arr in (rev[5], s0[5], s1[5], res[5].reversed, sc2[5], scr2[5]):
        assert arr.size == 24 and not arr.any()                               # zeros for the refused group
    for w in (0, 1, 2, 3, 4, 6):
        assert cons[w] == got[w].consensus and rev[w].tolist() == got[w].reversed.tolist() and int(status[w]) == capi.VC_WIN_OK, w
        assert s0[w].tolist() == sc[w].tolist() and s1[w].tolist() == scr[w].tolist() and res[w].rows == got[w].rows, w
    print(f"[degenerate groups] empty, empty-member and refused groups beside valid ones, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. the plain calls before and after, sharing the buffer cache
def test_plain_calls_unchanged_after_a_strand_call(built, monkeypatch, capfd):
    groups = _fresh(9800, 96)
    batch = poa.group_batch(groups)
    t0 = time.time()
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    monkeypatch.setenv("VC_LARGE_MAT_MB", "2")

    def plain():
        out = []
        for p in (capi.VcPoaGapParams(0, 1, 5, -4, -8, -8, -8, -8), capi.VcPoaGapParams(0, 2, 5, -4, -8, -6, -10, -4)):
            capfd.readouterr()
            cons, st = poa.run_batch(batch, p)
            e0 = capfd.readouterr().err
            res, st7 = poa.run_batch_msa(batch, p, 7)
            e7 = capfd.readouterr().err
            out.append((cons, st.tolist(), [(m.rows, m.members, m.consensus, m.coverage.tolist()) for m in res], st7.tolist(),
                        [l for l in e0.splitlines() if l.startswith("vc_large:")], [l for l in e7.splitlines() if l.startswith("vc_large:")]))
        return out
    try:
        before = plain()
        capfd.readouterr()
        res, st, _, _ = _strand(groups, 1, MODELS["convex"])
        es = capfd.readouterr().err
        after = plain()
    finally:
        monkeypatch.delenv("VC_LARGE_LOG")
        monkeypatch.delenv("VC_LARGE_MAT_MB")
    assert st.tolist() == [capi.VC_WIN_OK] * len(groups) and sum(int(m.reversed.sum()) for m in res) > 50
    assert before == after and all(len(_done("\n".join(b[4]))) == 1 for b in before)
    assert _done(es)[0][0] % 2 == 0 and _done(es)[0][0] > 0
    print(f"[plain calls beside the strand call] vc_poa_run_gaps and vc_poa_run_msa, bytes and log lines equal before and after, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 6. the command line
def test_command_line_on_the_sample_with_half_flipped(built, tmp_path):
    raw = gzip.open(os.path.join(GOLDEN, "sample.fastq.gz"), "rt").read().split("\n")
    names = [l[1:].split()[0] for l in raw[0::4] if l]
    seqs, quals = fixtures.load_sample_reads()
    es = {l: e for l, _, _, _, e in entries()}
    flips = es["GlobalWithQualities"]["flips"]
    fq = tmp_path / "flipped.fastq"
    with open(fq, "wb") as f:
        for nm, (s, q) in zip(names, flipped(list(zip(seqs, quals)), flips)):
            f.write(b"@%s\n%s\n+\n%s\n" % (nm.encode(), s, q))
    t0 = time.time()
    run = lambda *a: subprocess.run([sys.executable, "-m", "vechat_amd.poa", *a, str(fq)], cwd=ROOT, capture_output=True, timeout=300)  # noqa: E731
    for lvl, key in (("0", "LocalWithQualities"), ("1", "GlobalWithQualities"), ("2", "SemiGlobalWithQualities")):
        p = run("-l", lvl, "-r", "2", "--both-strands")
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout.decode() == "".join(f">{n}\n{row}\n" for n, row in zip(names + ["Consensus"], es[key]["rows"])), lvl
    e = es["GlobalWithQualities"]
    p = run("-l", "1", "--both-strands")
    assert p.returncode == 0 and p.stdout.decode() == f">Consensus LN:i:{len(e['consensus'])}\n{e['consensus']}\n"
    p = run("-l", "1", "--both-strands", "--coverage")
    assert p.returncode == 0 and p.stdout.decode() == (f">Consensus LN:i:{len(e['consensus'])} CV:B:I," + ",".join(map(str, e["coverage"]))
                                                       + f"\n{e['consensus']}\n")
    e = es["GlobalConvexWithQualities"]
    p = run("-l", "1", "--both-strands", "--gap-extend", "-6", "--gap-open2", "-10", "--gap-extend2", "-2")
    assert p.returncode == 0 and p.stdout.decode() == f">Consensus LN:i:{len(e['consensus'])}\n{e['consensus']}\n"
    print(f"[command line] --both-strands with -r 0 / -r 2, --coverage and convex gaps on the sample with every second read flipped, "
          f"{time.time() - t0:.1f} s")
