"""GPU suite (-m gpu): span-limited alignment of POA group members (vc_poa_run_spans, the spans= keyword of vechat_amd.poa) byte
for byte against spoa's own Subgraph / UpdateAlignment / AddAlignment loop -- every entry of tests/golden/poa_spans.json.gz, all
outputs, the three gap models, the strand flow --, one mixed batch, the regrowth that subgraph() can cause, the refusals before
the device, the log lines, and the windows the oracle already pins.  The shapes are the fixture's (backbones of at most 400
bases, at most 24 members): what can go wrong is which rows an alignment reads and how its pairs are mapped back, not size.
Each test prints its time."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import fixtures
import oracle_api as oa
import poa_graph_ref as G
from poa_common import MODELS, _done, _gp
from test_poa_align_gpu import _knobs
from test_poa_spans import NONE, SPAN_ERRORS, _members, _spans, check_entry, entries, load_spans_fixture
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
OK = capi.VC_WIN_OK
FLAGS = capi.VC_POA_MSA | capi.VC_POA_MSA_CONSENSUS | capi.VC_POA_COVERAGE


def _call(groups, spans, t, scores, strands=False):
    """one vc_poa_run_spans with rows, consensus row, coverage and graph tables (and the strand outputs) -> poa._Outputs"""
    return poa._run(poa.group_batch(groups), capi.VcPoaGapParams(0, t, *scores), msa_flags=FLAGS, strands=strands, graph=True,
                    spans=poa.span_arrays(groups, spans))


def _got(x, w):
    """group w of a call in the form check_entry reads"""
    g = x.graphs[w]
    m = g.msa
    d = dict(consensus=x.cons[w], rows=m.rows, members=m.members, coverage=m.coverage.tolist(), tables=G.of_poa_graph(g))
    if x.scores is not None:
        d.update(reversed=m.reversed.tolist(), score=x.scores[w].tolist(), score_rev=x.scores_rev[w].tolist())
    return d


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("strand", [False, True], ids=["plain", "strand"])
def test_every_fixture_entry_byte_for_byte(built, strand):
    """one call per (algorithm, score set): every group of the fixture that has it, all outputs at once"""
    t0 = time.time()
    calls = {}
    for e in entries():
        if e[5] == strand:
            calls.setdefault((e[3], e[4]), []).append(e)
    n = 0
    for (t, scores), es in sorted(calls.items()):
        x = _call([mem for _, mem, *_ in es], [spans for _, _, spans, *_ in es], t, scores, strands=strand)
        assert x.status.tolist() == [OK] * len(es)
        for w, (label, *_, want) in enumerate(es):
            check_entry(_got(x, w), want, label)
        n += len(es)
    assert n == (15 if strand else 96)
    print(f"[fixture, {'strand' if strand else 'plain'} flow] {n} entries in {len(calls)} calls: consensus, rows, members, coverage, graph tables"
          f"{', strand choices and scores' if strand else ''} equal to spoa's, {time.time() - t0:.1f} s")


def test_python_keywords_select_the_entry(built):
    """poa_consensus / poa_consensus_strands / poa_msa / poa_graph with spans= give the fixture's bytes too"""
    fx = load_spans_fixture()
    g = fx["seeded"][3]
    groups, spans, e = [_members(g["seqs"])], [_spans(g["spans"])], g["expected"]["1"]
    assert poa.poa_consensus(groups, "global", *g["scores"][:3], spans=spans) == [e["consensus"].encode()]
    m = poa.poa_msa(groups, "global", *g["scores"][:3], include_consensus=True, coverage=True, spans=spans)[0]
    assert m.consensus == e["consensus"].encode() and m.coverage.tolist() == e["coverage"] and len(m.rows) == e["n_rows"]
    gr = poa.poa_graph(groups, "global", *g["scores"][:3], spans=spans)[0]
    assert G.digest(G.of_poa_graph(gr)) == e["digest"]
    cons, rev = poa.poa_consensus_strands(groups, "global", *g["scores"][:3], spans=spans)
    assert cons == [e["consensus"].encode()] and not rev[0].any()
    assert G.digest(G.of_poa_graph(poa.poa_graph(groups, "global", *g["scores"][:3])[0])) != e["digest"]     # without spans: another graph


def test_command_line_with_spans(built, tmp_path, capfdbinary):
    """--spans FILE through main(): parse_spans, span_arrays and every call main() makes with the keyword -- the consensus, the rows
    with coverage, the graph -- on two fixture groups, against the fixture"""
    fx = load_spans_fixture()
    pick = [fx["seeded"][3], next(h for h in fx["hand"] if h["name"] == "repeat")]
    files, lines = [], []
    for k, g in enumerate(pick):
        path = tmp_path / f"group{k}.fasta"
        path.write_text("".join(f">m{i}\n{s}\n" for i, (s, _) in enumerate(g["seqs"])))
        files.append(str(path))
        lines += [f"{path}\tm{i}\t{sp[0]}\t{sp[1]}\n" for i, sp in enumerate(g["spans"]) if sp is not None]
    tsv = tmp_path / "spans.tsv"
    tsv.write_text("".join(reversed(lines)))
    # the fixture's seeded members carry qualities that a FASTA file does not: the expectation is the restatement's on the same bytes
    import poa_spans_ref as SR
    want = [SR.run([(s.encode(), None) for s, _ in g["seqs"]], _spans(g["spans"]), 1, 5, -4, -8) for g in pick]
    assert want[1]["consensus"].decode() == pick[1]["expected"]["1"]["consensus"]

    def run(*args):
        capfdbinary.readouterr()
        assert poa.main(["-l", "1", "--spans", str(tsv), *args, *files]) == 0
        return capfdbinary.readouterr().out
    assert run() == b"".join(b">Consensus LN:i:%d\n%s\n" % (len(w["consensus"]), w["consensus"]) for w in want)
    both = [SR.run([(s.encode(), None) for s, _ in g["seqs"]], _spans(g["spans"]), 1, 5, -4, -8, strands=True)["consensus"] for g in pick]
    assert run("--both-strands") == b"".join(b">Consensus LN:i:%d\n%s\n" % (len(c), c) for c in both)
    rows = run("-r", "2").split(b"\n")[1::2]
    assert rows == [r for w in want for r in w["rows"]]
    cov = run("--coverage").split(b"\n")[0::2]
    assert cov[:2] == [b">Consensus LN:i:%d CV:B:I%s" % (len(w["consensus"]), b"".join(b",%d" % c for c in w["coverage"])) for w in want]
    gfa = run("--gfa-consensus")
    plain = lambda *a: (capfdbinary.readouterr(), poa.main(["-l", "1", *a, *files]), capfdbinary.readouterr().out)[2]      # noqa: E731
    assert gfa != plain("--gfa-consensus") and gfa.count(b"\nP\t") == sum(len(g["seqs"]) + 1 for g in pick)
    graphs = poa.poa_graph([[(s.encode(), None) for s, _ in g["seqs"]] for g in pick], "global", 5, -4, -8, spans=[_spans(g["spans"]) for g in pick])
    assert gfa == b"".join(gr.to_gfa([f"m{i}" for i in range(len(g["seqs"]))], include_consensus=True) for gr, g in zip(graphs, pick))
    assert [G.of_poa_graph(gr) for gr in graphs] == [w["tables"] for w in want]


# ------------------------------------------------------------------ 2. one mixed batch
def test_span_groups_none_groups_and_an_empty_group_in_one_call(built):
    t0 = time.time()
    fx = load_spans_fixture()
    pick = [fx["seeded"][k] for k in (1, 5, 8, 10)] + [h for h in fx["hand"] if h["name"] in ("all_none", "empty_member_with_span", "repeat")]
    groups, spans, want = [], [], []
    for k, g in enumerate(pick):
        groups.append(_members(g["seqs"])); spans.append(_spans(g["spans"])); want.append(g["expected"]["1"])
        if k % 2 == 0:                                   # the same group without spans beside it: the plain call's bytes
            groups.append(_members(g["seqs"])); spans.append(None); want.append(None)
    groups.insert(3, []); spans.insert(3, None); want.insert(3, None)
    x = _call(groups, spans, 1, MODELS["linear"])
    assert x.status.tolist() == [OK] * len(groups)
    plain = poa._run(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *MODELS["linear"]), msa_flags=FLAGS, graph=True)
    for w, e in enumerate(want):
        if e is not None:
            check_entry(_got(x, w), e, f"group {w}")
        else:
            assert _got(x, w) == _got(plain, w), w
    assert x.cons[3] == b"" and x.graphs[3].n_nodes == 0
    print(f"[mixed batch] {len(groups)} groups -- with spans, without, empty -- in one call: the fixture's and the plain call's bytes, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 3. regrowth
def _grown(err):
    out = []
    for l in err.splitlines():
        if l.startswith("vc_large: regrow"):
            out.append(set(re.search(r"flags=(\S+)", l).group(1).split(",")))
    return out


def test_regrowth_from_the_subgraph_stack_and_from_every_table(built, monkeypatch, capfd):
    """VC_LARGE_CAPS is read on every call, so the small tables are set for single calls of this process.
    The stack: subgraph() leaves an entry behind for every branch it passes, so on seed10 (1 211 bases; global, linear) its stack
    reaches 80 entries while no topological sort of the build needs more than 6 (walked on the CPU restatement).  s:6 starts the
    stack at (4 x 1 211 + 129) >> 6 = 77 entries: it is subgraph() that fills it, exactly once (the doubled stack holds 80).
    The other tables: a subgraph's nodes, edges and aligned cells are subsets of the graph's and both slots have the same
    capacities, so those bits are always raised by the full graph first; the subgraph then works in the regrown tables."""
    t0 = time.time()
    g = load_spans_fixture()["seeded"][10]
    assert g["name"] == "seed10_len180_n15" and sum(len(s) for s, _ in g["seqs"]) == 1211
    groups, spans = [_members(g["seqs"])], [_spans(g["spans"])]
    x, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "s:6"}, lambda: _call(groups, spans, 1, MODELS["linear"]))
    assert _grown(err) == [{"stack"}], err
    assert x.status.tolist() == [OK]
    # the group ran twice, and every member with a span and a base is counted once all the same
    assert _spans_line(err)[0][0] == sum(1 for (s, _), sp in zip(groups[0][1:], spans[0][1:]) if sp is not None and s)
    check_entry(_got(x, 0), g["expected"]["1"], "stack regrown")
    y, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:3,e:3,a:6,l:3,p:4"}, lambda: _call(groups, spans, 1, MODELS["linear"]))
    grown = set().union(*_grown(err))
    assert {"nodes", "edges", "aligned", "labels", "pairs"} <= grown, grown
    assert y.status.tolist() == [OK]
    check_entry(_got(y, 0), g["expected"]["1"], "tables regrown")
    print(f"[regrowth] stack from subgraph() once, then {sorted(grown)}: the fixture's bytes both times, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("case", SPAN_ERRORS, ids=[c[0] for c in SPAN_ERRORS])
def test_bad_spans_are_refused_with_no_device_touched(built, monkeypatch, capfd, case):
    """the same refusals as on a machine without a device (tests/test_poa_spans.py), and nothing ran: a call that reaches the
    device ends with the `done` line, a refused one prints nothing"""
    _, begin, end, who, what = case
    lib = capi.load_hip()
    groups = [[b"ACGTACGTACGT", b"ACGTAC", b"GTACGT"], [b"ACGTACGT", b"ACGT"]]
    batch = poa.group_batch(groups)

    def run():
        cons, off, status, r, vb = poa._result_buffers(batch)
        sb, se = np.array(begin, np.uint32), np.array(end, np.uint32)
        sp = capi.VcPoaSpanIn(sb.ctypes.data_as(C.POINTER(C.c_uint32)), se.ctypes.data_as(C.POINTER(C.c_uint32)))
        return lib.vc_poa_run_spans(C.byref(_gp()), C.byref(sp), C.byref(vb), C.byref(r), None, None, None), lib.vc_poa_last_error().decode()
    (rc, msg), err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, run)
    assert rc == capi.VC_ERR_ARG and who in msg and what in msg, (rc, msg)
    assert "vc_large:" not in err, err


# ------------------------------------------------------------------ 5. the log lines
def _tiled(seed, locus=384, length=96, depth=3):
    rng = np.random.default_rng(seed)
    backbone = bytes(rng.choice(list(b"ACGT"), locus).tolist())
    mem, spans = [(backbone, None)], [None]
    for b in range(0, locus, length):
        for _ in range(depth):
            s = bytearray(backbone[b:b + length])
            for k in rng.choice(length, 4, replace=False):
                s[k] = b"ACGT"[(b"ACGT".index(s[k]) + 1) % 4]
            mem.append((bytes(s), None)); spans.append((b, b + length - 1))
    return mem, spans


def _spans_line(err):
    lines = [l for l in err.splitlines() if l.startswith("vc_large: spans")]
    return [tuple(map(int, re.match(r"vc_large: spans members=(\d+) sub_rows=(\d+) full_rows=(\d+)$", l).groups())) for l in lines]


def test_a_call_without_a_span_prints_the_parents_lines(built, monkeypatch, capfd):
    groups = [_tiled(1)[0], _tiled(2)[0]]
    batch, p = poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *MODELS["linear"])
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.25"}
    (old, _), err_old = _knobs(monkeypatch, capfd, env, lambda: poa.run_batch(batch, p))
    nb = np.full(len(batch.seq_off) - 1, NONE, np.uint32)
    for sp in (None, (nb, nb.copy())):                   # spans=None takes vc_poa_run_gaps; every entry NONE goes through the new entry
        new, err_new = _knobs(monkeypatch, capfd, env, lambda: poa._run(batch, p, spans=sp))
        assert new.cons == old and err_new == err_old
    assert not _spans_line(err_old) and len(_done(err_old)) == 1 and "step launches" in err_old


def test_the_spans_line_counts_members_and_rows(built, monkeypatch, capfd):
    t0 = time.time()
    mem, spans = _tiled(3)
    groups, sp = [mem, mem], [spans, None]
    x, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: poa._run(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *MODELS["linear"]),
                                                                               graph=True, spans=poa.span_arrays(groups, sp)))
    assert x.status.tolist() == [OK, OK]
    (m, sub_rows, full_rows), = _spans_line(err)
    assert m == len(mem) - 1 == 12 and sub_rows < full_rows
    assert sub_rows >= m * 96 and full_rows >= m * 384                     # a tile's subgraph holds its 96 backbone nodes at least
    assert sub_rows * 3 < full_rows                                        # four tiles: about a quarter of the rows
    (aligns, cells), = _done(err)
    assert aligns == 2 * (len(mem) - 1)
    # every tiled read lies on its own tile of the backbone; without spans the global alignment stretches it over the locus
    for k, (b, e) in enumerate(spans[1:], 1):
        path = next(p for mb, _, p in x.graphs[0].paths() if mb == k)
        on = [v for v in path if v < 384]
        assert on and b <= min(on) and max(on) <= e, k
    y, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: poa._run(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *MODELS["linear"]),
                                                                               strands=True, spans=poa.span_arrays(groups, sp)))
    assert _spans_line(err) == [(m, 2 * sub_rows, 2 * full_rows)] and y.cons == x.cons      # both strands' passes, the members once
    print(f"[spans line] members={m} sub_rows={sub_rows} full_rows={full_rows}, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 6. through the path the oracle already pins
def test_windows_through_the_span_entry_give_the_oracles_untrimmed_consensus(built):
    """tests/test_poa_spans.py says which windows of tests/golden/windows.json qualify and why; here the device runs them"""
    t0 = time.time()
    fx = fixtures.load_windows()
    batch = fixtures.fixture_batch(fx["windows"])
    p = capi.VcParams(**fx["params"])
    p.mode, p.trim = 1, 0
    cons, polished, _ = oa.oracle_run(batch, p)
    groups, spans, want = [], [], []
    for w in range(batch.n_windows):
        seqs, quals, b, e = batch.window(w)
        if len(seqs) < 3:
            continue
        s0 = int(batch.win_seq_off[w])
        groups.append([(bytes(s), bytes(q) if batch.seq_has_qual[s0 + k] else None) for k, (s, q) in enumerate(zip(seqs, quals))])
        spans.append(poa.racon_spans(len(seqs[0]), [None] + [(int(x), int(y)) for x, y in zip(b[1:], e[1:])]))
        want.append(cons[w])
    got = poa.poa_consensus(groups, "global", p.match, p.mismatch, p.gap, spans=spans)
    assert len(got) == 23 and got == want
    print(f"[windows] {len(got)} windows of the oracle's fixture through vc_poa_run_spans: the untrimmed mode-1 consensus, {time.time() - t0:.1f} s")
