"""GPU suite (-m gpu): queries aligned against the finished graphs of POA groups without being added (vc_poa_run_align,
poa.poa_align, the command line's --align) -- every entry of tests/golden/poa_align.json.gz byte for byte, freshly seeded groups
against the CPU restatement tests/poa_align_ref.py, invariants that need no model, the lane and chunk boundaries of the shared
row body, the host schedule under the development knobs, statuses, the calls without queries, and the command line.  Each test
prints its time."""
import os
import random
import re
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import poa_align_ref as A
from poa_strand_ref import reverse_complement
from poa_common import MODELS, _workers
from test_poa_align import entries
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, STRANDS = capi.VC_POA_ALIGN_PAIRS, capi.VC_POA_ALIGN_STRANDS
OK = capi.VC_WIN_OK


def _align(groups, queries, t, scores, flags=PAIRS, graph=False):
    """-> (consensus per group, group statuses, QueryAlignment lists, graphs or None)"""
    return poa.run_batch_align(poa.group_batch(groups), poa.query_batch(queries), capi.VcPoaGapParams(0, t, *scores), flags, graph=graph)


def _flat(res):
    return [(r.status, r.score, r.score_rev, r.reversed, None if r.pairs is None else r.pairs.tolist()) for qs in res for r in qs]


def _log(err):
    m = re.findall(r"vc_large: align jobs=(\d+) launches=(\d+) cells=(\d+) bytes=(\d+)", err)
    assert len(m) == 1, err
    return tuple(map(int, m[0]))


# ------------------------------------------------------------------ 1. every fixture entry
@pytest.mark.parametrize("part", range(6))
def test_every_fixture_entry(built, part):
    """the entries by engine (algorithm, scores), a call per engine and flag setting; the engines dealt over six cases"""
    t0 = time.time()
    calls = {}
    for label, mem, queries, squeries, t, scores, e in entries():
        calls.setdefault((t, scores), []).append((label, mem, queries, squeries, e))
    assert len(calls) >= 6
    calls = dict(sorted(calls.items())[part::6])
    n = 0
    for (t, scores), es in calls.items():
        for which, flags, qi in (("plain", PAIRS, 2), ("strand", PAIRS | STRANDS, 3)):
            _, status, res, _ = _align([x[1] for x in es], [x[qi] for x in es], t, scores, flags)
            assert status.tolist() == [OK] * len(es)
            for x, qs in zip(es, res):
                assert len(qs) == len(x[4][which]), x[0]
                for k, (r, want) in enumerate(zip(qs, x[4][which])):
                    assert r.status == OK and A.same(A.of_query_alignment(r), want), (x[0], which, k)
                    n += 1
    print(f"[fixture, part {part}] {n} alignments in {2 * len(calls)} calls: status, score, score_rev, reversed and pairs equal to spoa's, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. fresh groups against the restatement
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


def _fresh(seed, n):
    """n groups of 3 to 8 members of 30 to 150 bases at 6 % noise with 1 to 6 queries each: members, mutated members, random
    sequences and reverse complements, in turn"""
    rng = random.Random(seed)
    groups, queries = [], []
    for w in range(n):
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 151)))
        g = [(_noisy(rng, truth), None) for _ in range(rng.randrange(3, 9))]
        qs = []
        for k in range(rng.randrange(1, 7)):
            s = rng.choice(g)[0]
            kind = (w + k) % 4
            qs.append(s if kind == 0 else _noisy(rng, s, 0.15) if kind == 1 else
                      bytes(rng.choice(b"ACGT") for _ in range(len(s))) if kind == 2 else reverse_complement(_noisy(rng, s)))
        groups.append(g); queries.append(qs)
    return groups, queries


def _ref_job(a):
    g, qs, t, scores = a
    eng, gr = A.build(g, t, *scores)
    return [A.align_one(eng, gr, s, False) for s in qs], [A.align_one(eng, gr, s, True) for s in qs]


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("t", [0, 1, 2])
def test_fresh_groups_against_the_restatement(built, t, model):
    groups, queries = _fresh(8100 + 10 * t + list(MODELS).index(model), 100)
    scores = MODELS[model]
    t0 = time.time()
    plain = _align(groups, queries, t, scores, PAIRS)
    both = _align(groups, queries, t, scores, PAIRS | STRANDS)
    only = _align(groups, queries, t, scores, STRANDS)                      # the scores alone: no backtrack
    t1 = time.time()
    with ProcessPoolExecutor(_workers()) as ex:
        ref = list(ex.map(_ref_job, [(g, qs, t, scores) for g, qs in zip(groups, queries)], chunksize=4))
    n = n_rev = 0
    for w, (rp, rb) in enumerate(ref):
        for k in range(len(queries[w])):
            for got, want in ((plain[2][w][k], rp[k]), (both[2][w][k], rb[k])):
                assert got.status == OK and A.of_query_alignment(got) == want, (t, model, w, k)
            o, b = only[2][w][k], both[2][w][k]
            assert o.pairs is None and (o.score, o.score_rev, o.reversed) == (b.score, b.score_rev, b.reversed), (t, model, w, k)
            n += 1; n_rev += b.reversed
    assert plain[0] == both[0] == only[0] and n_rev > 20
    print(f"[fresh groups, algorithm {t}, {model} gaps] {n} queries of {len(groups)} groups, {n_rev} kept reversed: scores and pairs equal "
          f"to the restatement with and without strands; device {t1 - t0:.1f} s, restatement {time.time() - t1:.1f} s")


# ------------------------------------------------------------------ 3. invariants that need no model
@pytest.mark.parametrize("model", ["linear", "affine"])
def test_invariants_from_the_graph_of_the_same_call(built, model):
    groups, queries = _fresh(8200, 60)
    m, n, g, e, _, _ = MODELS[model]
    t0 = time.time()
    for t in (0, 1, 2):
        _, status, res, graphs = _align(groups, queries, t, MODELS[model], PAIRS, graph=True)
        assert status.tolist() == [OK] * len(groups)
        for w, (qs, gr) in enumerate(zip(res, graphs)):
            rank_of = np.empty(gr.n_nodes, np.int64)
            rank_of[gr.rank_to_node] = np.arange(gr.n_nodes)
            edges = {(a, b) for a, b, _ in gr.edges()}
            for k, r in enumerate(qs):
                pos = [p for _, p in r.pairs.tolist() if p != -1]
                nodes = [v for v, _ in r.pairs.tolist() if v != -1]
                assert pos == sorted(set(pos)) and all(0 <= v < gr.n_nodes for v in nodes), (t, w, k)
                assert all(rank_of[a] < rank_of[b] for a, b in zip(nodes, nodes[1:])), (t, w, k)
                if t == 1:
                    assert pos == list(range(len(queries[w][k]))), (t, w, k)
                    assert A.path_score(r.pairs.tolist(), queries[w][k], gr.node_base.tobytes(), edges, m, n, g, e) == r.score, (t, w, k)
    print(f"[invariants, {model} gaps] positions ascend (NW: each once), nodes ascend in rank order along edges, the NW score recomputed "
          f"from pairs, bases and gap model equals the reported one, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. lane and chunk boundaries of the shared row body
@pytest.mark.parametrize("model", list(MODELS))
def test_lane_and_chunk_boundaries(built, model):
    rng = random.Random(8300)
    truth = bytes(rng.choice(b"ACGT") for _ in range(60))
    group = [(_noisy(rng, truth), None) for _ in range(3)]
    long = (truth * 18)[:1025]
    queries = [_noisy(rng, long[:n], 0.03)[:n].ljust(n, b"A") for n in (1, 8, 9, 511, 512, 513, 1025)]
    assert [len(s) for s in queries] == [1, 8, 9, 511, 512, 513, 1025]
    t0 = time.time()
    for t in (0, 1, 2):
        _, _, res, _ = _align([group], [queries], t, MODELS[model], PAIRS | STRANDS)
        want = A.align_queries(group, queries, t, *MODELS[model], both_strands=True)
        for k, (r, x) in enumerate(zip(res[0], want)):
            assert r.status == OK and A.of_query_alignment(r) == x, (t, k)
    print(f"[boundaries, {model} gaps] query lengths 1, 8, 9, 511, 512, 513, 1025 against one small graph, three algorithms: equal to the "
          f"restatement, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. the host schedule
def _knobs(monkeypatch, capfd, env, f):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        capfd.readouterr()
        out = f()
        err = capfd.readouterr().err
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return out, err


def test_schedule_under_the_knobs(built, monkeypatch, capfd):
    groups, queries = _fresh(8400, 80)
    rng = random.Random(8401)
    big = bytes(rng.choice(b"ACGT") for _ in range(900))
    groups.append([(big, None), (_noisy(rng, big), None)]); queries.append([_noisy(rng, big), b"ACGT"])   # ~ 900 x 900 cells: above 0.25 MiB
    nq = sum(len(q) for q in queries)
    t0 = time.time()
    free, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _align(groups, queries, 1, MODELS["affine"], PAIRS))
    j0, k0, c0, b0 = _log(err)
    assert j0 == nq and k0 == 1 and b0 > 0
    # the done line keeps counting the build's passes only
    _, plain_err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: poa.run_batch(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *MODELS["affine"])))
    done = lambda e: re.findall(r"vc_large: done alignments=(\d+) cells=(\d+)", e)   # noqa: E731
    assert done(err) == done(plain_err) and len(done(err)) == 1
    # small matrices and arena: several launches, one of them a single job above the budget; several host groups
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.25", "VC_LARGE_ARENA_MB": "2"}
    tight, err = _knobs(monkeypatch, capfd, env, lambda: _align(groups, queries, 1, MODELS["affine"], PAIRS))
    j1, k1, c1, _ = _log(err)
    assert len(re.findall(r"vc_large: group windows=", err)) >= 2, "one host group only"
    assert (j1, c1) == (nq, c0) and k1 >= 4
    # the launches, from the job sizes alone: under the matrix budget only (one host group, so that the packing runs over all jobs
    # in order) the host must pack greedily -- consecutive jobs while their (rows + 1) x (length + 1) x 3 planes of int32 fit, at
    # least one -- and the long query, above the budget by itself, must sit in a launch of its own
    solo, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.25"},
                       lambda: _align(groups, queries, 1, MODELS["affine"], PAIRS, graph=True))
    budget, launches, fill = int(0.25 * 2 ** 20) // 4, [], 0
    for g, qs in zip(solo[3], queries):
        for s in qs:
            if not g.n_nodes or not s:
                continue
            need = (g.n_nodes + 1) * (len(s) + 1) * 3
            if launches and fill + need <= budget:
                launches[-1].append(need); fill += need
            else:
                launches.append([need]); fill = need
    over = [l for l in launches if sum(l) > budget]
    big = (solo[3][-1].n_nodes + 1) * (len(queries[-1][0]) + 1) * 3
    assert all(len(l) == 1 for l in over) and [big] in over and big > 30 * budget and any(len(l) > 1 for l in launches)
    assert len(re.findall(r"vc_large: group windows=", err)) == 1 and _log(err)[:3] == (nq, len(launches), c0)
    assert _flat(solo[2]) == _flat(free[2])
    assert _flat(tight[2]) == _flat(free[2]) and tight[0] == free[0]
    # both strands: exactly twice the cells
    both, err = _knobs(monkeypatch, capfd, env, lambda: _align(groups, queries, 1, MODELS["affine"], PAIRS | STRANDS))
    j2, k2, c2, _ = _log(err)
    assert (j2, c2) == (nq, 2 * c0) and k2 >= k1
    # regrown groups: their queries are counted once
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,s:10,p:6"}
    grown, err = _knobs(monkeypatch, capfd, env, lambda: _align(groups, queries, 1, MODELS["affine"], PAIRS))
    j3, _, c3, _ = _log(err)
    assert "vc_large: regrow" in err and (j3, c3) == (nq, c0)
    assert _flat(grown[2]) == _flat(free[2])
    print(f"[schedule] {nq} queries of {len(groups)} groups: {k0} launch unconstrained, {k1} under a 0.25 MiB matrix budget over several "
          f"host groups ({k2} with both strands, twice the cells), regrown groups' queries counted once; results equal, {time.time() - t0:.1f} s")


def test_every_output_stage_through_the_shared_launch_loop(built, monkeypatch, capfd):
    """The four stages that share the host's launch loop -- the build's alignment steps, the alignment rows, the graph tables and
    the queries -- in one process, every output asked for: vc_poa_run_graph with rows, coverage and strands, then
    vc_poa_run_align with pairs, both query strands, the build's strands and the graph.  Once without a knob, once with small
    tables (every group regrows), an arena of 0.5 MiB (several host groups of several groups each) and a matrix budget of 8 KiB
    (a group's rows are about 1 KiB, its graph block tens of KiB, a query matrix hundreds: launches of several items, of one
    item, and of one item above the budget).  Every table, row, score and pair must equal the knob-free call's."""
    import poa_graph_ref as G
    rng = random.Random(8450)
    groups, queries = [], []
    for w in range(24):
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 151)))
        g = [(_noisy(rng, truth), None) for _ in range(rng.randrange(2, 7))]
        if w % 3 == 0:
            g[-1] = (reverse_complement(g[-1][0]), None)
        groups.append(g)
        queries.append([g[0][0], _noisy(rng, truth, 0.15), reverse_complement(_noisy(rng, truth))])
    groups[7] = []                                                          # an empty group keeps its three queries
    batch, qbatch = poa.group_batch(groups), poa.query_batch(queries)
    p = capi.VcPoaGapParams(0, 1, *MODELS["convex"])

    def both():
        return (poa.run_batch_graph(batch, p, 7, strands=True),
                poa.run_batch_align(batch, qbatch, p, PAIRS | STRANDS, strands=True, graph=True))
    t0 = time.time()
    fg, fa = both()
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,l:3,s:10,p:6", "VC_LARGE_ARENA_MB": "0.5", "VC_LARGE_MAT_MB": "0.008"}
    (kg, ka), err = _knobs(monkeypatch, capfd, env, both)
    launches = {k: [int(x) for x in re.findall(rf"vc_large: {k} (?:jobs=\d+ )?launches=(\d+)", err)] for k in ("msa", "graph", "align")}
    print(f"[shared loop] launches {launches}, {err.count('vc_large: regrow')} regrow lines, "
          f"{err.count('vc_large: group windows=')} host groups, {err.count('vc_large: step launches=')} steps of several launches")
    assert "vc_large: regrow" in err and "vc_large: step launches=" in err
    assert len(launches["msa"]) == 1 and len(launches["graph"]) == 2 and len(launches["align"]) == 1      # one line per call that has the stage
    assert all(k >= 2 for ks in launches.values() for k in ks), launches
    for got, want in ((kg, fg), (ka, fa)):
        assert got[1].tolist() == want[1].tolist() == [OK] * len(groups)
    # vc_poa_run_graph: the tables, the rows and the coverage beside them, the strand choices and both strands' scores
    for w, (x, y) in enumerate(zip(kg[0], fg[0])):
        assert G.of_poa_graph(x) == G.of_poa_graph(y) and x.consensus == y.consensus, w
        assert (x.msa.rows, x.msa.members, x.msa.coverage.tolist(), x.msa.reversed.tolist()) == \
               (y.msa.rows, y.msa.members, y.msa.coverage.tolist(), y.msa.reversed.tolist()), w
        assert kg[2][w].tolist() == fg[2][w].tolist() and kg[3][w].tolist() == fg[3][w].tolist(), w
    # vc_poa_run_align: consensus, every query's status, scores, strand and pairs, the graph of the same call
    assert ka[0] == fa[0] and _flat(ka[2]) == _flat(fa[2]) and len(_flat(fa[2])) == 3 * len(groups)
    assert [G.of_poa_graph(x) for x in ka[3]] == [G.of_poa_graph(y) for y in fa[3]] == [G.of_poa_graph(y) for y in fg[0]]
    assert any(r.reversed for qs in fa[2] for r in qs) and any(m.msa.reversed.any() for m in fg[0])
    print(f"[shared loop] {len(groups)} groups, {3 * len(groups)} queries: tables, rows, coverage, scores and pairs under small tables, arena "
          f"and matrix budget equal to the knob-free calls, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 6. statuses
def test_a_group_that_is_not_computed_and_a_group_without_queries(built, monkeypatch, capfd):
    """No input of testable size makes the reference throw on a POA group, so -- as in the tests of vc_poa_run_msa, _strand and
    _graph -- the group that is not computed is one the arena budget refuses: its queries carry VC_WIN_OVERFLOW, score 0 and
    no pairs, and the rest of the batch is computed."""
    groups, queries = _fresh(8500, 30)
    rng = random.Random(8501)
    want = _align(groups, queries, 2, MODELS["linear"], PAIRS | STRANDS)
    big = [(bytes(rng.choice(b"ACGT") for _ in range(3000)), None) for _ in range(24)]
    g2 = groups[:10] + [big] + groups[10:]
    q2 = queries[:10] + [[b"ACGTACGT", b"", b"TTTT"]] + queries[10:]
    q2[3], q2[20] = [], []                                                  # groups without queries beside groups that have some
    t0 = time.time()
    got, _ = _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: _align(g2, q2, 2, MODELS["linear"], PAIRS | STRANDS))
    assert got[1].tolist() == [OK] * 10 + [capi.VC_WIN_OVERFLOW] + [OK] * 20
    assert _flat([got[2][10]]) == [(capi.VC_WIN_OVERFLOW, 0, 0, False, [])] * 3
    assert got[2][3] == [] and got[2][20] == []
    rest = got[2][:10] + got[2][11:]
    for w in range(30):
        if w not in (3, 19):
            assert _flat([rest[w]]) == _flat([want[2][w]]), w
    with pytest.raises(poa.PoaError):
        _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: poa.poa_align(g2, q2, 2))
    print(f"[statuses] a refused group's queries carry its status, groups without queries lie between: the rest equal to the call "
          f"without them, {time.time() - t0:.1f} s")


def test_a_call_whose_jobs_are_all_empty_allocates_nothing(built, monkeypatch, capfd):
    """Every job of the call is an empty alignment -- an empty query, or any query against the graph of an empty group -- so the job
    stage lists its jobs and stops before its device allocation: the log line counts the jobs and no launch, cell or byte.  Every
    query is VC_WIN_OK with the restatement's result (score 0, no pair), with one strand and with both."""
    groups, _ = _fresh(8550, 3)
    groups.append([])
    queries = [[b"", b""], [b""], [b"", b"", b""], [b"ACGTACGT", b""]]
    scores = MODELS["affine"]
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.01", "VC_LARGE_ARENA_MB": "0.5"}
    t0 = time.time()
    built_ = [A.build(g, 1, *scores) for g in groups]
    for flags, strands in ((PAIRS, False), (PAIRS | STRANDS, True)):
        got, err = _knobs(monkeypatch, capfd, env, lambda: _align(groups, queries, 1, scores, flags))
        assert _log(err) == (sum(len(qs) for qs in queries), 0, 0, 0) and sum(len(qs) for qs in queries) == 8, err
        assert got[1].tolist() == [OK] * 4 and got[0][3] == b"" and all(got[0][:3])
        for (eng, gr), qs, res in zip(built_, queries, got[2]):
            assert len(res) == len(qs)
            for s, r in zip(qs, res):
                assert r.status == OK and A.of_query_alignment(r) == A.align_one(eng, gr, s, strands), (flags, s)
    print(f"[empty jobs] 8 queries, every one an empty alignment: 8 jobs, no launch, no cell, no byte copied; equal to the restatement, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 7. calls without queries
def test_calls_without_queries_are_unchanged(built, monkeypatch, capfd):
    groups, queries = _fresh(8600, 24)
    batch = poa.group_batch(groups)
    p = capi.VcPoaGapParams(0, 1, *MODELS["convex"])
    monkeypatch.setenv("VC_LARGE_LOG", "1")

    def logged(f):
        capfd.readouterr()
        out = f()
        return out, capfd.readouterr().err
    try:
        before = [logged(f) for f in (lambda: poa.run_batch(batch, p), lambda: poa.run_batch_msa(batch, p, 7),
                                      lambda: poa.run_batch_msa(batch, p, 7, strands=True), lambda: poa.run_batch_graph(batch, p, 7))]
        with_q, err = logged(lambda: poa.run_batch_align(batch, poa.query_batch(queries), p, PAIRS | STRANDS, graph=True))
        assert "vc_large: align jobs=" in err
        none, err = logged(lambda: poa.run_batch_align(batch, poa.query_batch([[] for _ in groups]), p, PAIRS, graph=True))
        assert "vc_large: align" not in err and all(q == [] for q in none[2])
        after = [logged(f) for f in (lambda: poa.run_batch(batch, p), lambda: poa.run_batch_msa(batch, p, 7),
                                     lambda: poa.run_batch_msa(batch, p, 7, strands=True), lambda: poa.run_batch_graph(batch, p, 7))]
    finally:
        monkeypatch.delenv("VC_LARGE_LOG")
    import poa_graph_ref as G
    for (b, eb), (a, ea) in zip(before, after):
        assert "vc_large: align" not in eb + ea and eb == ea                # the same log: the same passes, launches and bytes
    assert before[0][0][0] == after[0][0][0] == with_q[0] == none[0]
    for k in (1, 2):
        assert [(m.rows, m.members, m.coverage.tolist()) for m in before[k][0][0]] == [(m.rows, m.members, m.coverage.tolist()) for m in after[k][0][0]]
    for x, y, z in zip(before[3][0][0], after[3][0][0], with_q[3]):
        assert G.of_poa_graph(x) == G.of_poa_graph(y) == G.of_poa_graph(z)
    print("[calls without queries] vc_poa_run_gaps, _msa, _strand and _graph give the same bytes and the same log before and after a call "
          "with queries, and log no align line; a call with an empty query batch runs no stage")


# ------------------------------------------------------------------ 8. the command line
def test_command_line(built, tmp_path):
    groups, queries = _fresh(8700, 2)
    files = []
    for w, g in enumerate(groups):
        files.append(str(tmp_path / f"group{w}.fasta"))
        with open(files[-1], "wb") as f:
            for i, (s, _) in enumerate(g):
                f.write(b">r%d\n%s\n" % (i, s))
    qs = queries[0] + queries[1]
    with open(tmp_path / "queries.fasta", "wb") as f:
        for i, s in enumerate(qs):
            f.write(b">q%d\n%s\n" % (i, s))
    t0 = time.time()
    out = tmp_path / "align.tsv"
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--align", str(tmp_path / "queries.fasta"), "--align-out", str(out),
                        "--align-both-strands", *files], cwd=ROOT, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    plain = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", *files], cwd=ROOT, capture_output=True, timeout=300)
    assert plain.returncode == 0 and p.stdout == plain.stdout                # the consensus output is unchanged
    want = []
    refs = [A.align_queries(g, qs, 1, 5, -4, -8, both_strands=True) for g in groups]
    for k in range(len(qs)):
        for w in range(2):
            r = refs[w][k]
            prs = ",".join(f"{'*' if v < 0 else v}:{'*' if x < 0 else x}" for v, x in r["pairs"]) or "*"
            want.append(f"q{k}\t{files[w]}\tOK\t{r['score_rev'] if r['reversed'] else r['score']}\t{'-' if r['reversed'] else '+'}\t{prs}\n")
    assert out.read_bytes() == "".join(want).encode()
    print(f"[command line] --align / --align-out / --align-both-strands on two group files and {len(qs)} queries: the restatement's "
          f"lines, stdout unchanged, {time.time() - t0:.1f} s")
