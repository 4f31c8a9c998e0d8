"""GPU suite (-m gpu): the partial order graph of POA groups (vc_poa_run_graph, poa.poa_graph, the command line's --gfa /
--gfa-consensus / --graphviz) table for table against spoa's own graph and byte for byte against its command line's text -- every
entry of tests/golden/poa_graph.json.gz --, freshly seeded groups against the CPU restatement tests/poa_graph_ref.py, in the plain
and in the strand flow, the calls that already exist on the same groups, every table regrown, many groups over several output
launches with an empty and a refused group among them, the old calls' launch sequence, and the command line.  Each test prints its
time."""
import os
import random
import re
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import pytest

import fixtures
import poa_graph_ref as G
from poa_common import MODELS, _kw, _workers
from test_poa import members
from test_poa_graph import check_graph, entries, load_graph_fixture, same_text, sample_names
from test_poa_strand import flipped
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graphs(groups, t, scores, flags=0, strands=False):
    return poa.run_batch_graph(poa.group_batch(groups), capi.VcPoaGapParams(0, t, *scores), flags, strands=strands)


# ------------------------------------------------------------------ 1. every fixture entry
def test_every_fixture_entry(built):
    t0 = time.time()
    calls = {}
    for label, mem, names, t, scores, strand, e in entries():
        calls.setdefault((t, scores, strand), []).append((label, mem, names, e))
    n = 0
    for (t, scores, strand), es in calls.items():
        got, status = _graphs([mem for _, mem, _, _ in es], t, scores, strands=strand)[:2]
        assert status.tolist() == [capi.VC_WIN_OK] * len(es)
        for (label, mem, names, e), g in zip(es, got):
            check_graph(G.of_poa_graph(g), e, names, label)                  # counts, digest, tables, and the text of to_gfa / to_dot
            if "text" in e:
                assert same_text(g.to_gfa(names, include_consensus=True), e["text"]["gfa_consensus"]) and same_text(g.to_dot(), e["text"]["dot"])
            n += 1
    print(f"[fixture] {n} graphs in {len(calls)} calls: every table equal to spoa's, GFA and dot text equal to its command line's, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. fresh groups against the restatement, and the calls that exist
def _noisy(rng, s, rate=0.06):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= x < rate:
            out.append(rng.choice(b"ACGT"))
    return bytes(out) or s[:1]


def _fresh(seed, n, flips):
    """n groups of 2 to 12 members of 30 to 150 bases at 6 % noise, a third of the groups with qualities; flips: members
    reverse-complemented at random"""
    rng = random.Random(seed)
    out = []
    for w in range(n):
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 151)))
        g = []
        for _ in range(rng.randrange(2, 13)):
            s = _noisy(rng, truth)
            g.append((s, bytes(33 + rng.randrange(2, 40) for _ in s) if w % 3 == 1 else None))
        out.append(flipped(g, [k for k in range(len(g)) if rng.random() < 0.5]) if flips else g)
    return out


def _ref_job(a):
    g, t, scores, strands = a
    return G.graph(g, t, *scores, strands=strands)


@pytest.mark.parametrize("strands", [False, True], ids=["plain", "strand"])
@pytest.mark.parametrize("t", [0, 1, 2])
def test_fresh_groups_against_the_restatement_and_the_existing_calls(built, t, strands):
    groups = _fresh(7100 + 10 * t + strands, 100, strands)
    model_of = [list(MODELS)[(w // 3) % 3] for w in range(len(groups))]
    t0 = time.time()
    got, n_rev = [None] * len(groups), 0
    for model, scores in MODELS.items():
        idx = [w for w in range(len(groups)) if model_of[w] == model]
        sub = [groups[w] for w in idx]
        p = capi.VcPoaGapParams(0, t, *scores)
        res = _graphs(sub, t, scores, 7, strands)
        assert res[1].tolist() == [capi.VC_WIN_OK] * len(sub)
        # the calls that already exist, on the same groups
        cons = poa.run_batch(poa.group_batch(sub), p)[0] if not strands else None
        old = poa.run_batch_msa(poa.group_batch(sub), p, 7, strands=strands)
        for k, (w, g, m) in enumerate(zip(idx, res[0], old[0])):
            assert g.consensus == m.consensus and (strands or g.consensus == cons[k]), (t, w)
            assert (g.msa.rows, g.msa.members, g.msa.coverage.tolist()) == (m.rows, m.members, m.coverage.tolist()), (t, w)   # the MSA of the same call
            base = g.node_base.tobytes()
            for (mb, rev, path), row, rm in zip(g.paths(), m.rows, m.members):
                assert mb == rm and bytes(base[v] for v in path) == row.replace(b"-", b""), (t, w, mb)
            if strands:
                assert g.msa.reversed.tolist() == m.reversed.tolist() and res[2][k].tolist() == old[2][k].tolist() \
                    and res[3][k].tolist() == old[3][k].tolist(), (t, w)
                assert [r for _, r, _ in g.paths()] == [bool(m.reversed[mb]) for mb, _, _ in g.paths()], (t, w)
                n_rev += int(m.reversed.sum())
            got[w] = g
    t1 = time.time()
    with ProcessPoolExecutor(_workers()) as ex:
        ref = list(ex.map(_ref_job, [(g, t, MODELS[model_of[w]], strands) for w, g in enumerate(groups)], chunksize=4))
    for w, (g, r) in enumerate(zip(got, ref)):
        have = G.of_poa_graph(g)
        for k in r:
            assert have[k] == r[k], (t, w, k)
    assert not strands or n_rev > 100
    print(f"[fresh groups, algorithm {t}, {'strand' if strands else 'plain'} flow] {len(groups)} groups over linear / affine / convex gaps"
          f"{f', {n_rev} members kept reversed' if strands else ''}: every table equal to the restatement; consensus, rows, strands and "
          f"scores equal to the existing calls; device {t1 - t0:.1f} s, restatement {time.time() - t1:.1f} s")


# ------------------------------------------------------------------ 3. every table regrown
def _hand():
    return [members(g) for g in load_graph_fixture()["hand"]]


def test_every_table_regrown(built, monkeypatch, capfd):
    """VC_LARGE_CAPS is read on every call, so the small tables are set for one call of this process, as the tests of the other
    vc_poa_* calls do"""
    groups = _hand() + _fresh(7200, 40, True)
    want, st = _graphs(groups, 1, MODELS["affine"], 7, True)[:2]
    assert st.tolist() == [capi.VC_WIN_OK] * len(groups)
    env = (("VC_LARGE_CAPS", "n:5,e:5,a:7,l:3,s:10,p:6"), ("VC_LARGE_LOG", "1"))
    for k, v in env:
        monkeypatch.setenv(k, v)
    t0 = time.time()
    try:
        capfd.readouterr()
        got, st = _graphs(groups, 1, MODELS["affine"], 7, True)[:2]
        err = capfd.readouterr().err
    finally:
        for k, _ in env:
            monkeypatch.delenv(k)
    grown = set()
    for l in err.splitlines():
        if l.startswith("vc_large: regrow"):
            grown |= set(re.search(r"flags=(\S+)", l).group(1).split(","))
    assert grown == {"nodes", "edges", "aligned", "labels", "stack", "pairs"}, grown
    assert st.tolist() == [capi.VC_WIN_OK] * len(groups)
    for w, (a, b) in enumerate(zip(got, want)):
        assert G.of_poa_graph(a) == G.of_poa_graph(b) and a.msa.rows == b.msa.rows, w
    print(f"[regrowth] {len(groups)} groups, the hand-made boundary groups among them, every table regrown ({sorted(grown)}): the same "
          f"tables, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. many groups over several output launches
def test_many_small_groups_over_several_launches_with_an_empty_and_a_refused_group(built, monkeypatch, capfd):
    """No input of testable size makes the reference throw on a POA group (VC_WIN_INVALID needs a worst-case score beyond int32), so the
    group that is not computed is one the arena budget refuses, VC_WIN_OVERFLOW, as in the tests of vc_poa_run_msa and
    vc_poa_run_strand: it has zero counts, and its neighbours are intact."""
    rng = random.Random(7300)
    small = _fresh(7301, 298, False)
    big = [(bytes(rng.choice(b"ACGT") for _ in range(3000)), None) for _ in range(24)]
    groups = small[:100] + [[]] + small[100:200] + [big] + small[200:]
    alone = _graphs(small, 2, MODELS["linear"])[0]
    for k, v in (("VC_LARGE_ARENA_MB", "4"), ("VC_LARGE_MAT_MB", "0.25"), ("VC_LARGE_LOG", "1")):
        monkeypatch.setenv(k, v)
    t0 = time.time()
    try:
        capfd.readouterr()
        got, st = _graphs(groups, 2, MODELS["linear"])
        err = capfd.readouterr().err
        with pytest.raises(poa.PoaError) as ex:
            poa.poa_graph(groups, 2)
        loose = poa.poa_graph(groups, 2, strict=False)
    finally:
        for k in ("VC_LARGE_ARENA_MB", "VC_LARGE_MAT_MB", "VC_LARGE_LOG"):
            monkeypatch.delenv(k)
    k, nbytes = map(int, re.search(r"vc_large: graph launches=(\d+) bytes=(\d+)", err).groups())
    assert k >= 3 and nbytes > 0
    assert ex.value.groups == {201: capi.VC_WIN_OVERFLOW} and loose[201] is None and loose[100] is not None
    assert [int(s) for s in st] == [capi.VC_WIN_OK] * 201 + [capi.VC_WIN_OVERFLOW] + [capi.VC_WIN_OK] * 98
    for w in (100, 201):                                                   # the empty and the refused group: zero counts
        assert G.counts(G.of_poa_graph(got[w])) == [0, 0, 0, 0, 0] and got[w].cons_node.size == 0 and got[w].out_off.tolist() == [0], w
    rest = got[:100] + got[101:201] + got[202:]
    for w, (a, b) in enumerate(zip(rest, alone)):
        assert G.of_poa_graph(a) == G.of_poa_graph(b), w
    print(f"[many groups] {len(groups)} groups in {k} output launches, {nbytes} bytes copied out, an empty and a refused group with zero "
          f"counts between intact neighbours, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. the old calls launch no new kernel
def test_old_calls_launch_no_graph_kernel(built, monkeypatch, capfd):
    groups = _fresh(7400, 24, True)
    batch = poa.group_batch(groups)
    p = capi.VcPoaGapParams(0, 1, *MODELS["convex"])
    monkeypatch.setenv("VC_LARGE_LOG", "1")

    def launches(f):
        capfd.readouterr()
        f()
        m = re.findall(r"vc_large: graph launches=(\d+) bytes=(\d+)", capfd.readouterr().err)
        return sum(int(k) for k, _ in m)
    try:
        assert launches(lambda: poa.run_batch(batch, capi.VcPoaParams(0, 1, 5, -4, -8))) == 0                 # vc_poa_run
        assert launches(lambda: poa.run_batch(batch, p)) == 0                                                # vc_poa_run_gaps
        assert launches(lambda: poa.run_batch_msa(batch, p, 7)) == 0                                         # vc_poa_run_msa
        assert launches(lambda: poa.run_batch_msa(batch, p, 7, strands=True)) == 0                           # vc_poa_run_strand
        assert launches(lambda: poa.run_batch_graph(batch, p)) >= 1
        assert launches(lambda: poa.run_batch_graph(batch, p, 7, strands=True)) >= 1
        assert launches(lambda: poa.run_batch_msa(batch, p, 7)) == 0                                         # and none after it either
    finally:
        monkeypatch.delenv("VC_LARGE_LOG")
    print("[old calls] vc_poa_run, _gaps, _msa and _strand launch no graph kernel; vc_poa_run_graph does")


# ------------------------------------------------------------------ 6. the command line
def test_command_line_on_the_sample(built, tmp_path):
    """The sample's reads as FASTA, with their names: the first read's quality string is all '!', which the project's reader
    counts as none and spoa's as weights of 0, so on the FASTQ itself the two command lines differ by design (vechat_amd/poa.py)
    and the fixture records no text for it.  Against the recorded text of the known answer `Global`: plain, and with every second
    read flipped and --both-strands."""
    seqs, _ = fixtures.load_sample_reads()
    kat = load_graph_fixture()["kat"]["Global"]
    mem = [(s, None) for s in seqs]
    t0 = time.time()
    for which, group, extra in (("plain", mem, []), ("strand", flipped(mem, kat["flips"]), ["--both-strands"])):
        fa, dot = tmp_path / f"{which}.fasta", tmp_path / f"{which}.dot"
        with open(fa, "wb") as f:
            for nm, (s, _) in zip(sample_names(), group):
                f.write(b">%s\n%s\n" % (nm.encode(), s))
        p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "--gfa-consensus", "-l", "1", *extra, "--graphviz", str(dot), str(fa)],
                           cwd=ROOT, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        assert same_text(p.stdout, kat[which]["text"]["gfa_consensus"]) and same_text(dot.read_bytes(), kat[which]["text"]["dot"]), which
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "--gfa", "-l", "1", str(tmp_path / "plain.fasta")], cwd=ROOT,
                       capture_output=True, timeout=300)
    assert p.returncode == 0 and same_text(p.stdout, kat["plain"]["text"]["gfa"])
    print(f"[command line] --gfa, --gfa-consensus and --graphviz, plain and with --both-strands, equal to spoa's -r 3 / -r 4 / -s / -d, "
          f"{time.time() - t0:.1f} s")
