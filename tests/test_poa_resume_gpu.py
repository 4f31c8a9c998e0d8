"""GPU suite (-m gpu): POA groups that go on from a stored graph (vc_poa_run_from, poa.poa_extend, poa.poa_align(graphs=...), the
command line's --save-graphs / --from-graphs).  The contract under test: the tables and the state after members 0 .. k - 1,
passed back with members k .. n - 1 and the same parameters, give byte for byte what one call on all members gives.  Small
shapes: what can go wrong in k_lg_load is list order, carries past a tile of 64, regrowth and the empty cases, not size.
Each test prints its time."""
import os
import random
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import poa_align_ref as A
import poa_resume_ref as R
from poa_strand_ref import reverse_complement
from poa_common import MODELS
from test_poa import load_fixture, members
from test_poa_align import entries as align_entries
from test_poa_align_gpu import _flat, _knobs, _noisy
from test_poa_msa import load_msa_fixture
from test_poa_strand import entries as strand_entries
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = capi.VC_WIN_OK
FLAGS = capi.VC_POA_MSA | capi.VC_POA_MSA_CONSENSUS | capi.VC_POA_COVERAGE
PAIRS, STRANDS = capi.VC_POA_ALIGN_PAIRS, capi.VC_POA_ALIGN_STRANDS


def _p(t, scores):
    return capi.VcPoaGapParams(0, t, *scores)


def _call(groups, t, scores, start=None, **kw):
    """one vc_poa_run_from with rows, consensus row, coverage, graph tables and state -> poa._Outputs"""
    kw.setdefault("msa_flags", FLAGS)
    x = poa._run(poa.group_batch(groups), _p(t, scores), graph=True, state=True, start=start, **kw)
    assert x.status.tolist() == [OK] * len(groups)
    return x


def _all(x, w):
    """everything a call hands out for group w, in comparable form"""
    g = x.graphs[w]
    m = g.msa
    return (x.cons[w], R.of_poa_graph(g), None if m is None else (m.rows, m.members, m.coverage.tolist()))


# ------------------------------------------------------------------ 1. every split
def _splits(cases, t, scores):
    """cases: [(label, members)].  Three calls: every prefix of every group from nothing, every suffix on its prefix's graph, and
    every group whole; every split must give the whole group's bytes."""
    pre, suf, of = [], [], []
    for c, (_, mem) in enumerate(cases):
        for k in range(len(mem) + 1):
            pre.append(mem[:k]); suf.append(mem[k:]); of.append(c)
    whole = _call([mem for _, mem in cases], t, scores)
    first = _call(pre, t, scores)
    second = _call(suf, t, scores, start=first.graphs)
    for i, c in enumerate(of):
        assert _all(second, i) == _all(whole, c), (cases[c][0], t, len(pre[i]))
        assert first.graphs[i].n_members == len(pre[i]) and second.graphs[i].n_members == len(cases[c][1])
    return len(pre)


@pytest.mark.parametrize("t", [0, 1, 2])
def test_every_split_of_the_seeded_groups(built, t):
    t0 = time.time()
    by_scores = {}
    for g in load_fixture()["groups"]:
        if g["expected"][str(t)]["status"] == OK:
            by_scores.setdefault(tuple(g["scores"]), []).append((g["name"], members(g)))
    assert sum(len(v) for v in by_scores.values()) >= 28
    n = sum(_splits(cases, t, (m, x, gp, gp, gp, gp)) for (m, x, gp), cases in by_scores.items())
    print(f"[every split, algorithm {t}] {n} splits of {sum(len(v) for v in by_scores.values())} seeded groups: consensus, rows, coverage, "
          f"graph tables, state and members equal to the one call, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("model", ["affine", "convex"])
def test_every_split_with_affine_and_convex_gaps(built, model):
    t0 = time.time()
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    names = [g["name"] for g in load_msa_fixture()["gaps"] if g["model"] == model]
    assert len(names) == 5
    n = sum(_splits([(nm, groups[nm]) for nm in names], t, MODELS[model]) for t in (0, 1, 2))
    print(f"[every split, {model} gaps] {n} splits of five groups x three algorithms equal to the one call, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. chain, 3. identity
def _group(seed, n, length, rate=0.06):
    rng = random.Random(seed)
    truth = bytes(rng.choice(b"ACGT") for _ in range(length))
    return [(_noisy(rng, truth, rate), None) for _ in range(n)]


def test_chain_of_three_hops(built):
    t0 = time.time()
    groups = [_group(9100 + w, 8, 30 + 11 * w) for w in range(8)]
    for t, model in ((1, "linear"), (0, "affine"), (2, "convex")):
        whole = _call(groups, t, MODELS[model])
        x = _call([g[:2] for g in groups], t, MODELS[model])
        x = _call([g[2:5] for g in groups], t, MODELS[model], start=x.graphs)
        x = _call([g[5:] for g in groups], t, MODELS[model], start=x.graphs)
        assert [_all(x, w) for w in range(8)] == [_all(whole, w) for w in range(8)], (t, model)
    # the engine may differ between the hops, as in spoa: the result is the restatement's with the same engines
    x = _call([g[:4] for g in groups], 1, MODELS["linear"], msa_flags=None)
    x = _call([g[4:] for g in groups], 2, MODELS["affine"], start=x.graphs)
    for w, g in enumerate(groups):
        ref = R.build(g[4:], 2, MODELS["affine"], R.build(g[:4], 1, MODELS["linear"]))
        assert R.of_poa_graph(x.graphs[w]) == R.state(ref) and x.graphs[w].msa.rows == R.outputs(ref)[1], w
    print(f"[chain] 2 + 3 + 3 members over three calls equal to the one call (three engines); a change of engine between two hops "
          f"equal to the restatement, {time.time() - t0:.1f} s")


def test_load_and_export_is_the_identity(built, monkeypatch, capfd):
    t0 = time.time()
    groups = [_group(9200, 5, 80), [], [(b"", None), (b"", None)], _group(9201, 1, 1), _group(9202, 3, 70, 0.2)]
    first = _call(groups, 1, MODELS["convex"])
    assert first.graphs[1].n_nodes == first.graphs[2].n_nodes == 0 and [g.n_members for g in first.graphs] == [5, 0, 2, 1, 3]
    again, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _call([[] for _ in groups], 1, MODELS["convex"], start=first.graphs))
    assert [_all(again, w) for w in range(5)] == [_all(first, w) for w in range(5)]
    for a, b in zip(first.graphs, again.graphs):
        for k, _ in poa.PoaGraph._ARRAYS:
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    nodes, edges, paths = (sum(x) for x in zip(*[(g.n_nodes, g.edge_head.size, g.path_member.size) for g in first.graphs]))
    m = re.findall(r"vc_large: load groups=(\d+) nodes=(\d+) edges=(\d+) paths=(\d+) bytes=(\d+)", err)
    assert len(m) == 1 and tuple(map(int, m[0][:4])) == (5, nodes, edges, paths) and "done alignments=0 cells=0" in err
    # without labels (no rows, no graph): the consensus alone
    cons = poa._run(poa.group_batch([[] for _ in groups]), _p(1, MODELS["convex"]), start=first.graphs).cons
    assert cons == first.cons
    print(f"[identity] five stored graphs (one empty, one of empty members only) loaded and exported with no new member: every table "
          f"byte for byte, and the consensus without labels, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. tiles
def test_paths_and_lists_beyond_a_tile(built):
    t0 = time.time()
    rng = random.Random(9300)
    truth = bytes(rng.choice(b"ACGT") for _ in range(200))
    big = [(_noisy(rng, truth, 0.15), None) for _ in range(6)]
    big = [(s[:200] + truth[len(s[:200]):200], None) for s, _ in big]       # 6 members of 200 bases at 15 %
    exact = [(truth[:64], None), (truth[:65], None), (truth[1:65], None)]   # paths of exactly 64, 65 and 64 nodes
    assert [len(s) for s, _ in big] == [200] * 6 and [len(s) for s, _ in exact] == [64, 65, 64]
    cases = [("big", big), ("exact", exact)]
    n = 0
    for t, model in ((1, "linear"), (0, "convex")):
        n += _splits(cases, t, MODELS[model])
    g = _call([big], 1, MODELS["linear"]).graphs[0]
    indeg = np.bincount(g.edge_head, minlength=g.n_nodes)
    assert np.diff(g.path_off).min() > 128 and max(len(a) for a in g.aligned_lists) > 1 and indeg.max() > 1 and g.n_nodes > 256
    print(f"[tiles] {n} splits: paths of 200, 64 and 65 nodes, aligned classes up to {1 + max(len(a) for a in g.aligned_lists)} nodes, "
          f"in-degrees up to {indeg.max()}, {g.n_nodes} nodes: equal to the one call, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. strand flow
@pytest.mark.parametrize("t", [0, 1, 2])
def test_strand_flow_split_at_the_middle(built, t):
    """every entry of the strand fixture with this algorithm, known answers included, none left out: a call per engine"""
    t0 = time.time()
    by_engine = {}
    for label, mem, tt, scores, e in strand_entries():
        if tt == t:
            by_engine.setdefault((t, scores), []).append((label, mem))
    n = n_rev = 0
    for (t, scores), cases in sorted(by_engine.items()):
        groups = [mem for _, mem in cases]
        half = [len(g) // 2 for g in groups]
        whole = _call(groups, t, scores, strands=True)
        first = _call([g[:h] for g, h in zip(groups, half)], t, scores, strands=True)
        second = _call([g[h:] for g, h in zip(groups, half)], t, scores, strands=True, start=first.graphs)
        for w, h in enumerate(half):
            assert _all(second, w) == _all(whole, w), (cases[w][0], t)
            for got, want in ((second.scores, whole.scores), (second.scores_rev, whole.scores_rev)):
                assert got[w].tolist() == want[w][h:].tolist(), (cases[w][0], t)
            assert second.graphs[w].msa.reversed.tolist() == whole.graphs[w].msa.reversed[h:].tolist()
            kept = {int(m): bool(r) for m, r in zip(first.graphs[w].path_member, first.graphs[w].path_reversed)}
            after = {int(m): bool(r) for m, r in zip(second.graphs[w].path_member, second.graphs[w].path_reversed)}
            assert all(after[m] == r for m, r in kept.items())             # path_reversed of the earlier members is kept
            n += 1; n_rev += sum(kept.values())
    assert n >= 50 and n_rev > 0
    print(f"[strands, algorithm {t}] all {n} groups of the strand fixture split at the middle with the strand flow on both hops: reversed and scores equal "
          f"the tail of the one call's, {n_rev} earlier reversed paths kept, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 6. queries against stored graphs
@pytest.mark.parametrize("part", range(3))
def test_queries_against_stored_graphs(built, monkeypatch, capfd, part):
    t0 = time.time()
    by_engine = {}
    for label, mem, queries, squeries, t, scores, e in align_entries():
        by_engine.setdefault((t, scores), []).append((label, mem, queries, squeries, e))
    n = 0
    for (t, scores), es in sorted(by_engine.items())[part::3]:
        stored = poa._run(poa.group_batch([x[1] for x in es]), _p(t, scores), graph=True, state=True).graphs
        for which, flags, qi in (("plain", PAIRS, 2), ("strand", PAIRS | STRANDS, 3)):
            def run():
                return poa._run(poa.group_batch([[] for _ in es]), _p(t, scores), qbatch=poa.query_batch([x[qi] for x in es]),
                                align_flags=flags, start=stored)
            x, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, run)
            assert x.status.tolist() == [OK] * len(es)
            assert "vc_large: load groups=%d " % len(es) in err and "vc_large: done alignments=0 cells=0" in err
            for e, qs in zip(es, x.queries):
                assert len(qs) == len(e[4][which]), e[0]
                for k, (r, want) in enumerate(zip(qs, e[4][which])):
                    assert r.status == OK and A.same(A.of_query_alignment(r), want), (e[0], which, k)
                    n += 1
    print(f"[queries, part {part}] {n} alignments against stored graphs, no build in the call (0 alignments in the done line): status, scores, "
          f"strands and pairs equal to spoa's, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 7. regrowth
def test_regrowth_after_the_load(built, monkeypatch, capfd):
    t0 = time.time()
    groups = [_group(9400 + w, 8, 60 + 7 * w, 0.1) for w in range(12)]
    whole = _call(groups, 1, MODELS["affine"])
    first = _call([g[:3] for g in groups], 1, MODELS["affine"])
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,l:3,s:10,p:6", "VC_LARGE_ARENA_MB": "0.5"}
    second, err = _knobs(monkeypatch, capfd, env, lambda: _call([g[3:] for g in groups], 1, MODELS["affine"], start=first.graphs))
    assert [_all(second, w) for w in range(12)] == [_all(whole, w) for w in range(12)]
    regrown = {int(w) for w in re.findall(r"vc_large: regrow window=(\d+)", err)}
    ran = [int(w) for l in re.findall(r"vc_large: group windows=\d+ bytes=\d+ ids=([\d,]+)", err) for w in l.split(",")]
    assert regrown and all(ran.count(w) >= 2 for w in regrown) and len(re.findall(r"vc_large: load ", err)) == 1
    print(f"[regrowth] {len(regrown)} of 12 groups regrew their tables after the load and ran again from it ({len(ran)} group runs): "
          f"the one call's bytes, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 8. unchanged calls
def test_calls_without_from_and_state_are_the_present_ones(built, monkeypatch, capfd):
    t0 = time.time()
    groups = [_group(9500 + w, 5, 90) for w in range(6)]
    queries = [[g[0][0], _noisy(random.Random(w), g[1][0], 0.1)] for w, g in enumerate(groups)]
    batch, qbatch, p = poa.group_batch(groups), poa.query_batch(queries), _p(1, MODELS["affine"])
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.05"}
    lib = capi.load_hip()

    def through_from(with_queries):
        # from == NULL and st == NULL, through the new entry itself
        import ctypes as C
        cons, off, status, r, vb = poa._result_buffers(batch)
        g, o = capi.VcPoaGraphOut(), capi.VcPoaMsaOut(flags=FLAGS if not with_queries else 0)
        qv, a = qbatch.as_struct(), capi.VcPoaAlignOut(flags=PAIRS)
        rc = lib.vc_poa_run_from(C.byref(p), None, C.byref(vb), C.byref(r), None if with_queries else C.byref(o), None, C.byref(g), None,
                                 C.byref(qv) if with_queries else None, C.byref(a) if with_queries else None)
        assert rc == 0, lib.vc_poa_last_error()
        graphs = poa._graph_results(g, batch.n_windows, cons, off)
        return [R.G.of_poa_graph(x) for x in graphs], int(g.bytes), _flat(poa._query_results(a, PAIRS, [int(k) for k in qbatch.win_seq_off])) if with_queries else None

    (old_g, _), err_old_g = _knobs(monkeypatch, capfd, env, lambda: poa.run_batch_graph(batch, p, FLAGS))
    new_g, err_new_g = _knobs(monkeypatch, capfd, env, lambda: through_from(False))
    old_a, err_old_a = _knobs(monkeypatch, capfd, env, lambda: poa.run_batch_align(batch, qbatch, p, PAIRS, graph=True))
    new_a, err_new_a = _knobs(monkeypatch, capfd, env, lambda: through_from(True))
    assert err_new_g == err_old_g and err_new_a == err_old_a and "vc_large: graph launches=" in err_old_g
    assert "vc_large: load" not in err_new_g + err_new_a
    assert new_g[0] == [R.G.of_poa_graph(x) for x in old_g] and new_a[0] == [R.G.of_poa_graph(x) for x in old_a[3]]
    assert new_a[2] == _flat(old_a[2])
    # with the state the block grows by exactly the state table, and the tables beside it stay the same
    with_st, err_st = _knobs(monkeypatch, capfd, env, lambda: _call(groups, 1, MODELS["affine"]))
    b0 = int(re.search(r"vc_large: graph launches=\d+ bytes=(\d+)", err_old_g).group(1))
    b1 = int(re.search(r"vc_large: graph launches=\d+ bytes=(\d+)", err_st).group(1))
    extra = sum((4 * (g.n_nodes + 1) + 15) // 16 * 16 + (4 * g.al_node.size + 15) // 16 * 16 for g in with_st.graphs)
    assert "vc_large: state" not in err_new_g + err_new_a and int(re.search(r"vc_large: state bytes=(\d+)", err_st).group(1)) == extra
    assert b1 == b0 == new_g[1] and [R.G.of_poa_graph(x) for x in with_st.graphs] == new_g[0]
    print(f"[unchanged] vc_poa_run_graph and vc_poa_run_align beside vc_poa_run_from(from = NULL, st = NULL): the same tables, pairs and "
          f"log lines, no load line; the state adds {extra} bytes behind the blocks, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 9. command line
def test_command_line(built, tmp_path):
    t0 = time.time()
    groups = [_group(9600, 6, 70), _group(9601, 5, 90)]
    rng = random.Random(9602)
    qs = [groups[0][0][0], _noisy(rng, groups[1][1][0], 0.15), reverse_complement(groups[0][2][0])]

    def fasta(name, recs, tag):
        with open(tmp_path / name, "wb") as f:
            for i, s in enumerate(recs):
                f.write(b">%s%d\n%s\n" % (tag, i, s))
        return str(tmp_path / name)
    files = [fasta(f"group{w}.fasta", [s for s, _ in g], b"r") for w, g in enumerate(groups)]
    heads = [fasta(f"head{w}.fasta", [s for s, _ in g[:3]], b"r") for w, g in enumerate(groups)]
    tails = [fasta(f"tail{w}.fasta", [s for s, _ in g[3:]], b"r") for w, g in enumerate(groups)]
    q = fasta("queries.fasta", qs, b"q")

    def run(*args):
        p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", *args], cwd=ROOT, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout
    one = run("--align", q, "--align-out", str(tmp_path / "one.tsv"), "--align-both-strands", *files)
    saved = run("--save-graphs", str(tmp_path / "all.npz"), *files)
    again = run("--from-graphs", str(tmp_path / "all.npz"), "--align", q, "--align-out", str(tmp_path / "two.tsv"), "--align-both-strands")
    assert one == saved == again                                             # the consensus on stdout, with and without a build
    assert (tmp_path / "two.tsv").read_bytes() == (tmp_path / "one.tsv").read_bytes() != b""
    # extended on the way: three records, then the rest, then the queries; the files of the last hop name the groups
    run("--save-graphs", str(tmp_path / "head.npz"), *heads)
    ext = run("--from-graphs", str(tmp_path / "head.npz"), "--save-graphs", str(tmp_path / "ext.npz"), "--align", q,
              "--align-out", str(tmp_path / "three.tsv"), "--align-both-strands", *tails)
    assert ext == one
    want = (tmp_path / "one.tsv").read_bytes()
    for f, tl in zip(files, tails):
        want = want.replace(f.encode(), tl.encode())
    assert (tmp_path / "three.tsv").read_bytes() == want
    a, b = poa.PoaGraph.load(str(tmp_path / "ext.npz")), poa.PoaGraph.load(str(tmp_path / "all.npz"))
    assert [R.of_poa_graph(x) for x in a] == [R.of_poa_graph(x) for x in b]
    print(f"[command line] --save-graphs, then --from-graphs --align with no build and with the rest of the records added: the one-shot "
          f"run's consensus and --align-out lines, the same stored graphs, {time.time() - t0:.1f} s")
