"""GPU suite: queries assigned to POA groups on the device (vc_poa_run_assign, poa.poa_assign, --assign): every pair's score from
the ring of live rows (k_lg_slots, k_lg_sfwd) and the best and second group per query (k_lg_assign), against spoa's recorded
scores (tests/golden/poa_assign.json.gz), against the path the project already pins (vc_poa_run_align without pairs, the
queries repeated in every group), on hand shapes, under small budgets, from stored graphs and through the command line.

Not covered on the device: a pair that is VC_WIN_INVALID.  WorstCaseAlignmentScore falls below spoa's floor only beyond
128 x (query + rows) > 2^31, about 16 million rows with int8 scores and queries below 65 535 bases -- the same finding as in
tests/test_poa_align_gpu.py --, so the INVALID branch of status[k] is held by the restatement's test alone; the group that is not
VC_WIN_OK (refused by the arena budget) exercises the same fold with VC_WIN_OVERFLOW."""
import os
import random
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import poa_assign_ref as AR
from poa_common import MODELS, _kw
from test_poa_assign import entries, expected_assignments
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRANDS, SCORES = capi.VC_POA_ASSIGN_STRANDS, capi.VC_POA_ASSIGN_SCORES
OK = capi.VC_WIN_OK
ALGO = {0: "local", 1: "global", 2: "semi-global"}


def _assign(groups, queries, t, scores, flags=SCORES, start=None):
    """-> (consensus per group, group statuses, Assignments, score table, pair status table)"""
    return poa.run_batch_assign(poa.group_batch(groups), poa.query_batch([list(queries)]), capi.VcPoaGapParams(0, t, *scores), flags, start=start)


def _tuples(res):
    return [tuple(r) for r in res]


def _via_align(groups, queries, t, scores, strands):
    """the route the project already pins: vc_poa_run_align without pairs, every query placed in every group -> (kept scores
    [k][w], kept strands, statuses, group statuses)"""
    flags = capi.VC_POA_ALIGN_STRANDS if strands else 0
    _, gst, res, _ = poa.run_batch_align(poa.group_batch(groups), poa.query_batch([list(queries)] * len(groups)), capi.VcPoaGapParams(0, t, *scores), flags)
    nq = len(queries)
    kept = [[(res[w][k].score_rev if res[w][k].reversed else res[w][k].score) for w in range(len(groups))] for k in range(nq)]
    rev = [[res[w][k].reversed for w in range(len(groups))] for k in range(nq)]
    st = [[res[w][k].status for w in range(len(groups))] for k in range(nq)]
    return kept, rev, st, gst


def _same_as_align(groups, queries, t, scores, strands, got=None):
    kept, rev, st, gst = _via_align(groups, queries, t, scores, strands)
    cons, gst2, res, table, pst = got or _assign(groups, queries, t, scores, SCORES | (STRANDS if strands else 0))
    assert gst.tolist() == gst2.tolist()
    assert table.tolist() == kept and pst.tolist() == st
    has_node = [any(len(s) for s, _ in g) for g in groups]
    want = AR.assign(kept, st, has_node)
    assert [(r.best_group, r.best_score, r.second_group, r.second_score, r.status) for r in res] == want
    assert [r.reversed for r in res] == [bool(rev[k][r.best_group]) if r.best_group >= 0 else False for k, r in enumerate(res)]
    return res, table


def _log(err):
    m = re.findall(r"vc_large: assign groups=(\d+) queries=(\d+) pairs=(\d+) launches=(\d+) slots_max=(\d+) ring_cells=(\d+) full_cells=(\d+)", err)
    assert len(m) == 1, err
    return dict(zip(("groups", "queries", "pairs", "launches", "slots_max", "ring_cells", "full_cells"), map(int, m[0])))


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


def _noisy(rng, s, rate=0.08):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= x < rate:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def _families(seed, n, length=120, depth=5):
    rng = random.Random(seed)
    groups = []
    for _ in range(n):
        base = bytes(rng.choice(b"ACGT") for _ in range(length + rng.randint(-10, 10)))
        groups.append([(base, None)] + [(_noisy(rng, base), None) for _ in range(depth - 1)])
    queries = [_noisy(rng, rng.choice(g)[0]) for g in groups for _ in range(2)] + [bytes(rng.choice(b"ACGT") for _ in range(70)), b""]
    return groups, queries


def _hand_groups():
    """the hand graphs of the CPU test built as groups, an empty graph among them, one group twice, and a longer family"""
    rng = random.Random(9100)
    base = bytes(rng.choice(b"ACGT") for _ in range(600))
    names = sorted(AR.HAND_GROUPS)
    groups = [[(s, None) for s in AR.HAND_GROUPS[n]] for n in names]
    groups.insert(2, [])                                                        # an empty graph among real ones
    groups.append([(s, None) for s in AR.HAND_GROUPS["one_bubble"]])            # two identical groups
    groups.append([(base, None), (_noisy(rng, base), None), (_noisy(rng, base), None)])
    # 0, 1, 511, 512, 513 and 1 025 bases: a chunk is 64 lanes x 8 columns
    queries = [b"", b"A"] + [_noisy(rng, base)[:n] if n <= 560 else bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (511, 512, 513, 1025)]
    queries += [AR.HAND_GROUPS["one_bubble"][1], AR.HAND_GROUPS["skip_edge_first_to_last"][0], b"GGKACGTACGT", b"FFFFFFFF"]
    return names, groups, queries


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("index", range(8))
def test_every_fixture_entry(built, index):
    t0 = time.time()
    assert len(entries()) == 8
    name, groups, queries, scores, exp = entries()[index]
    for t in (0, 1, 2):
        for strands in (False, True):
            table, rev, ranks = expected_assignments(groups, exp[str(t)]["pairs"], strands)
            _, gst, res, got, pst = _assign(groups, queries, t, scores, SCORES | (STRANDS if strands else 0))
            assert gst.tolist() == [OK] * len(groups) and not pst.any()
            assert got.tolist() == table, (name, t, strands)
            assert [(r.best_group, r.best_score, r.second_group, r.second_score) for r in res] == ranks, (name, t, strands)
            assert [r.reversed for r in res] == [bg >= 0 and rev[k][bg] for k, (bg, _, _, _) in enumerate(ranks)], (name, t, strands)
            assert all(r.status == OK for r in res)
            # the Python call, and the call without the dense table
            if t == 1:
                plain = poa.poa_assign(groups, queries, both_strands=strands, algorithm=ALGO[t], **_kw(scores))
                assert _tuples(plain) == _tuples(res)
    print(f"[fixture] {name}: {len(queries)} queries x {len(groups)} groups, three algorithms, one strand and both: scores, best, second "
          f"and strand equal to spoa's, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. + 3. against vc_poa_run_align without pairs, on the hand shapes
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("t", (0, 1, 2))
def test_equal_to_align_without_pairs(built, t, model):
    t0 = time.time()
    names, groups, queries = _hand_groups()
    for strands in (False, True):
        res, table = _same_as_align(groups, queries, t, MODELS[model], strands)
        empty, twin_a, twin_b = 2, names.index("one_bubble") + 1, len(groups) - 2
        assert groups[empty] == [] and groups[twin_a] == groups[twin_b]
        assert not table[:, empty].any() and all(r.best_group != empty and r.second_group != empty for r in res)    # scored, never ranked
        assert (table[:, twin_a] == table[:, twin_b]).all()
        k = 6                                                                   # the bubble's own member: best is the lower index, second has the same score
        assert queries[k] == AR.HAND_GROUPS["one_bubble"][1]
        assert (res[k].best_group, res[k].second_group, res[k].second_score) == (twin_a, twin_b, res[k].best_score) and res[k].best_score == 50
    name, fg, fq, _, _ = entries()[0]
    for strands in (False, True):
        _same_as_align(fg, fq, t, MODELS[model], strands)
    print(f"[against align] algorithm {t}, {model} gaps: {len(queries)} queries of 0 .. 1 025 bases x {len(groups)} hand groups and the fixture's "
          f"families, one strand and both: equal to vc_poa_run_align without pairs, {time.time() - t0:.1f} s")


def test_twin_groups_tie_to_the_lower_index(built):
    g = [(s, None) for s in AR.HAND_GROUPS["one_bubble"]]
    other = [(b"TTTTTTTTTT", None)]
    for t in (0, 1, 2):
        res = poa.poa_assign([other, g, g], [AR.HAND_GROUPS["one_bubble"][0]], algorithm=ALGO[t])
        assert (res[0].best_group, res[0].second_group) == (1, 2) and res[0].best_score == res[0].second_score == 50


def test_a_group_that_is_not_computed(built, monkeypatch, capfd):
    """the group that is not VC_WIN_OK is one the arena budget refuses (as in tests/test_poa_align_gpu.py): its pairs carry its
    status and score 0, it is never ranked, every query is VC_WIN_OVERFLOW, and the ranked pairs are reported all the same"""
    groups, queries = _families(9200, 6)
    rng = random.Random(9201)
    big = [(bytes(rng.choice(b"ACGT") for _ in range(3000)), None) for _ in range(24)]
    want = _assign(groups, queries, 1, MODELS["linear"], SCORES | STRANDS)
    g2 = groups[:3] + [big] + groups[3:]
    got, _ = _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: _assign(g2, queries, 1, MODELS["linear"], SCORES | STRANDS))
    assert got[1].tolist() == [OK] * 3 + [capi.VC_WIN_OVERFLOW] + [OK] * 3
    assert not got[3][:, 3].any() and (got[4][:, 3] == capi.VC_WIN_OVERFLOW).all() and not np.delete(got[4], 3, axis=1).any()
    assert np.delete(got[3], 3, axis=1).tolist() == want[3].tolist()
    shift = lambda w: w + 1 if w >= 3 else w                                     # noqa: E731
    assert [(shift(a.best_group), a.best_score, shift(a.second_group), a.second_score, a.reversed) for a in want[2]] == \
        [(b.best_group, b.best_score, b.second_group, b.second_score, b.reversed) for b in got[2]]
    assert all(b.status == capi.VC_WIN_OVERFLOW for b in got[2]) and all(a.status == OK for a in want[2])
    with pytest.raises(poa.PoaError):
        _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: poa.poa_assign(g2, queries))


# ------------------------------------------------------------------ 4. the log line
@pytest.mark.parametrize("name", sorted(AR.HAND_GROUPS))
def test_log_line_counts_the_slots_of_the_hand_graphs(built, monkeypatch, capfd, name):
    group = [(s, None) for s in AR.HAND_GROUPS[name]]
    graph = poa.poa_graph([group])[0]
    preds = AR.rows_of(graph)
    slot, n_slots = AR.slots(preds)
    AR.check_slots(preds, slot, n_slots)
    queries = [b"ACGTACGT", b"AT", b""]
    got, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign([group], queries, 1, MODELS["linear"]))
    log = _log(err)
    print(f"[log] {name}: rows={len(preds)} n_slots={n_slots} {log}")
    assert (log["groups"], log["queries"], log["pairs"], log["launches"]) == (1, 3, 3, 1)
    assert log["slots_max"] == n_slots
    # the shapes are the CPU test's (longer chains and columns, which the rule does not count): the same n_slots
    assert n_slots == AR.HAND_ROWS[name][1], (name, n_slots)
    cols = sum(len(q) + 1 for q in queries if q)
    assert log["ring_cells"] == n_slots * cols and log["full_cells"] == (len(preds) + 1) * cols
    if len(preds) + 1 > n_slots:
        assert log["ring_cells"] < log["full_cells"]


# ------------------------------------------------------------------ 5. small budgets
def test_small_budgets_give_the_same_bytes_in_more_launches(built, monkeypatch, capfd):
    groups, queries = _families(9300, 12, length=300)
    flags = SCORES | STRANDS
    free, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign(groups, queries, 1, MODELS["affine"], flags))
    log0 = _log(err)
    assert log0["launches"] == 1 and err.count("vc_large: group windows=") == 1
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.05", "VC_LARGE_ARENA_MB": "1"}
    tight, err = _knobs(monkeypatch, capfd, env, lambda: _assign(groups, queries, 1, MODELS["affine"], flags))
    log1 = _log(err)
    assert err.count("vc_large: group windows=") > 1 and log1["launches"] > log0["launches"] + 2
    assert {k: log1[k] for k in ("pairs", "slots_max", "ring_cells", "full_cells")} == {k: log0[k] for k in ("pairs", "slots_max", "ring_cells", "full_cells")}
    assert free[0] == tight[0] and free[1].tolist() == tight[1].tolist() and _tuples(free[2]) == _tuples(tight[2])
    assert free[3].tobytes() == tight[3].tobytes() and free[4].tobytes() == tight[4].tobytes()
    # tables that regrow: the groups come back in another order, and the fold does not depend on it
    grown, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,s:10,p:6", "VC_LARGE_ARENA_MB": "1"},
                        lambda: _assign(groups, queries, 1, MODELS["affine"], flags))
    assert "vc_large: regrow" in err and _tuples(grown[2]) == _tuples(free[2]) and grown[3].tobytes() == free[3].tobytes()
    print(f"[budgets] {log0['pairs']} pairs: {log0['launches']} launch free, {log1['launches']} under 0.05 MiB of rings and 1 MiB of tables; "
          f"ring_cells / full_cells = {log0['ring_cells']} / {log0['full_cells']}")


# ------------------------------------------------------------------ 6. stored graphs
def test_stored_graphs_give_the_call_that_built_them(built):
    groups, queries = _families(9400, 5)
    want = _assign(groups, queries, 2, MODELS["convex"], SCORES | STRANDS)
    kw = dict(algorithm="semi-global", **_kw(MODELS["convex"]))
    stored = poa.poa_graph(groups, resumable=True, **kw)
    res, table = poa.poa_assign(graphs=stored, queries=queries, both_strands=True, scores=True, **kw)
    assert _tuples(res) == _tuples(want[2]) and table.tobytes() == want[3].tobytes()
    # built in two steps: three members, then poa_extend with the rest; and the rest added by the assign call itself
    first = poa.poa_graph([g[:3] for g in groups], resumable=True, **kw)
    extended, _ = poa.poa_extend(first, [g[3:] for g in groups], **kw)
    res2, table2 = poa.poa_assign(graphs=extended, queries=queries, both_strands=True, scores=True, **kw)
    res3, table3 = poa.poa_assign([g[3:] for g in groups], queries, graphs=first, both_strands=True, scores=True, **kw)
    assert _tuples(res2) == _tuples(res3) == _tuples(res) and table2.tobytes() == table3.tobytes() == table.tobytes()


# ------------------------------------------------------------------ 7. nothing to do
def test_no_queries_or_no_groups_run_no_stage(built, monkeypatch, capfd):
    groups, queries = _families(9500, 3)
    for flags in (0, STRANDS | SCORES):
        (cons, gst, res, table, pst), err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign(groups, [], 1, MODELS["linear"], flags))
        assert "vc_large: assign" not in err and "vc_large: done" in err and res == [] and all(cons) and gst.tolist() == [OK] * 3
        assert (table is None and pst is None) if not flags else (table.shape == pst.shape == (0, 3))
        (cons, gst, res, table, pst), err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign([], queries, 1, MODELS["linear"], flags))
        assert "vc_large:" not in err and cons == [] and _tuples(res) == [(-1, 0, -1, 0, False, OK)] * len(queries)
        assert (table is None) if not flags else (table.shape == pst.shape == (len(queries), 0))
    # groups that are all empty: a stage runs, every pair scores 0 and nothing is ranked
    (_, gst, res, table, pst), err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign([[], [(b"", None)]], queries, 1, MODELS["linear"], SCORES))
    assert _log(err)["launches"] == 0 and not table.any() and not pst.any() and _tuples(res) == [(-1, 0, -1, 0, False, OK)] * len(queries)


# ------------------------------------------------------------------ 8. the command line
def test_command_line(built, tmp_path):
    groups, queries = _families(9600, 2)
    files = []
    for w, g in enumerate(groups):
        files.append(str(tmp_path / f"group{w}.fasta"))
        with open(files[-1], "wb") as f:
            for i, (s, _) in enumerate(g):
                f.write(b">r%d\n%s\n" % (i, s))
    queries = [q for q in queries if q]
    with open(tmp_path / "queries.fasta", "wb") as f:
        for i, s in enumerate(queries):
            f.write(b">q%d\n%s\n" % (i, s))
    out, tab = tmp_path / "assign.tsv", tmp_path / "scores.tsv"
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--assign", str(tmp_path / "queries.fasta"), "--assign-out", str(out),
                        "--assign-both-strands", "--assign-scores", str(tab), *files], cwd=ROOT, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    plain = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", *files], cwd=ROOT, capture_output=True, timeout=300)
    assert plain.returncode == 0 and p.stdout == plain.stdout                   # the consensus output is unchanged
    res, table = poa.poa_assign(groups, queries, both_strands=True, scores=True)
    names = [b"q%d" % i for i in range(len(queries))]
    assert out.read_bytes() == poa.assign_tsv(names, files, res) and tab.read_bytes() == poa.assign_scores_tsv(names, files, table)
    assert len(out.read_bytes().splitlines()) == len(queries) and {r.best_group for r in res} == {0, 1}
    # with --from-graphs: the stored graphs, nothing added
    store = tmp_path / "graphs.npz"
    s = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--save-graphs", str(store), *files], cwd=ROOT, capture_output=True, timeout=300)
    assert s.returncode == 0, s.stderr.decode()
    out2 = tmp_path / "assign2.tsv"
    f = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--from-graphs", str(store), "--assign", str(tmp_path / "queries.fasta"),
                        "--assign-out", str(out2), "--assign-both-strands"], cwd=ROOT, capture_output=True, timeout=300)
    assert f.returncode == 0, f.stderr.decode()
    assert out2.read_bytes() == out.read_bytes()


# ------------------------------------------------------------------ 9. the existing path
def test_align_calls_log_what_they_logged(built, monkeypatch, capfd):
    """a vc_poa_run_align call prints the same vc_large: lines before and after an assign call, none of them an assign line, and
    returns the same bytes; the lines are the parent's: group, align, done"""
    groups, queries = _families(9700, 6)
    qs = [queries] * len(groups)
    p = capi.VcPoaGapParams(0, 1, *MODELS["convex"])
    run = lambda: poa.run_batch_align(poa.group_batch(groups), poa.query_batch(qs), p, capi.VC_POA_ALIGN_PAIRS | capi.VC_POA_ALIGN_STRANDS)  # noqa: E731
    flat = lambda r: [(x.status, x.score, x.score_rev, x.reversed, x.pairs.tolist()) for q in r[2] for x in q]                             # noqa: E731
    before, eb = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, run)
    _, ea = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _assign(groups, queries, 1, MODELS["convex"], SCORES | STRANDS))
    after, ec = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, run)
    assert eb == ec and "assign" not in eb and "vc_large: assign" in ea and "vc_large: align" not in ea
    assert [l.split()[1] for l in eb.splitlines() if l.startswith("vc_large:")] == ["group", "align", "done"]
    assert re.search(r"vc_large: align jobs=%d launches=1 cells=\d+ bytes=\d+\n" % (len(queries) * len(groups)), eb)
    assert before[0] == after[0] and flat(before) == flat(after)
