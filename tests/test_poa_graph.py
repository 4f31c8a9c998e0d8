"""CPU suite: the partial order graph of POA groups (vc_poa_run_graph, poa.poa_graph, PoaGraph.to_gfa / to_dot, the command
line's --gfa / --gfa-consensus / --graphviz) at its boundary -- declared, exported and bound with the documented layout, the
arguments refused before the device, the parser -- and the CPU restatement tests/poa_graph_ref.py, the live bar for the device,
against every entry of tests/golden/poa_graph.json.gz (spoa's own graph and its own command line's text)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import poa_graph_ref as G
import poa_strand_ref as S
from poa_common import TYPES, _gp, _workers
from test_poa import _device_visible, load_fixture, members
from test_poa_strand import flipped
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_FX = {}


def load_graph_fixture():
    if not _FX:
        _FX.update(json.load(gzip.open(os.path.join(GOLDEN, "poa_graph.json.gz"), "rt")))
    return _FX


def sample_names():
    raw = gzip.open(os.path.join(GOLDEN, "sample.fastq.gz"), "rt").read().split("\n")
    return [l[1:].split()[0] for l in raw[0::4] if l]


def entries():
    """every graph of the fixture -> [(label, members as passed to the call, names, algorithm, (m, n, g, e, q, c), strand, expected)]"""
    fx = load_graph_fixture()
    seqs, quals = fixtures.load_sample_reads()
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    out = []

    def both(label, mem, names, t, scores, flips, e):
        out.append((label + "/plain", mem, names, t, scores, False, e["plain"]))
        out.append((label + "/strand", flipped(mem, flips), names, t, scores, True, e["strand"]))
    for name, k in fx["kat"].items():
        both(name, list(zip(seqs, quals if k["quality"] else [None] * len(seqs))), sample_names(), TYPES[k["type"]], tuple(k["scores"]),
             k["flips"], k)
    for sec in ("groups", "gaps", "hand"):
        for g in fx[sec]:
            mem = members(g) if sec == "hand" else groups[g["name"]]
            sc = tuple(g["scores"]) if len(g["scores"]) == 6 else (g["scores"][0], g["scores"][1]) + (g["scores"][2],) * 4
            names = [f"{'read' if sec == 'hand' else 'r'}{i}" for i in range(len(mem))]
            for t in ("0", "1", "2"):
                both(f"{sec}/{g['name']}/{g.get('model', 'linear')}/{t}", mem, names, int(t), sc, g["flips"], g["expected"][t])
    return out


def same_text(got, rec):
    """bytes against a recorded text: its length and SHA-256, and the text itself where the fixture keeps it"""
    return len(got) == rec["bytes"] and hashlib.sha256(got).hexdigest() == rec["sha256"] and \
        ("text" not in rec or got == rec["text"].encode("latin-1"))


def check_graph(t, e, names, label):
    """tables (poa_graph_ref form) against a fixture graph: counts, digest, the tables where kept, the text where recorded"""
    assert G.counts(t) == e["counts"], (label, G.counts(t), e["counts"])
    if "tables" in e:
        want = G.unpack(e["tables"])
        for k in want:
            assert t[k] == want[k], (label, k)
    assert G.digest(t) == e["digest"], label
    if "text" in e:
        pg = G.to_poa_graph(t)
        if "gfa" in e["text"]:
            assert same_text(pg.to_gfa(names), e["text"]["gfa"]), label
        assert same_text(pg.to_gfa(names, include_consensus=True), e["text"]["gfa_consensus"]), label
        assert same_text(pg.to_dot(), e["text"]["dot"]), label


# ------------------------------------------------------------------ the boundary
def test_graph_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_graph" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_graph_out" in hdr and "The id rule" in hdr and "has no path" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_graph")
    body = hdr[hdr.index("typedef struct vc_poa_graph_out"):hdr.index("} vc_poa_graph_out;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in capi.VcPoaGraphOut._fields_]
    assert C.sizeof(capi.VcPoaGraphOut) == 152 and capi.VcPoaGraphOut.n_nodes.offset == 8 and capi.VcPoaGraphOut.bytes.offset == 144
    assert capi.load_hip().vc_poa_run_graph.argtypes[3:] == [C.POINTER(capi.VcPoaMsaOut), C.POINTER(capi.VcPoaStrandOut),
                                                             C.POINTER(capi.VcPoaGraphOut)]
    assert C.sizeof(capi.VcPoaMsaOut) == 72 and C.sizeof(capi.VcPoaStrandOut) == 24 and C.sizeof(capi.VcPoaGapParams) == 32   # unchanged


def _call(lib, params, batch, flags=0, out=True, strand="none", graph=True, **override):
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in override.items():
        setattr(vb, k, v)
    o = capi.VcPoaMsaOut(flags=flags)
    n = max(int(batch.win_seq_off[-1]) if batch.n_windows else 0, 1)
    rev = np.zeros(n, np.uint8)
    s = capi.VcPoaStrandOut()
    if strand == "all":
        s.reversed = rev.ctypes.data_as(C.POINTER(C.c_uint8))
    g = capi.VcPoaGraphOut()
    g.n_nodes = C.cast(1, C.POINTER(C.c_uint32))                               # a failed call must leave every pointer NULL
    rc = lib.vc_poa_run_graph(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r), C.byref(o) if out else None,
                              C.byref(s) if strand != "none" else None, C.byref(g) if graph else None)
    return rc, g


def test_graph_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad = [("null params", lambda: _call(lib, None, b)),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b)),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b)),
           ("gap_extend2 > 0", lambda: _call(lib, _gp(gap_extend2=2), b)),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b)),
           ("unknown flag bit 8", lambda: _call(lib, _gp(), b, 8)),
           ("consensus row without the MSA", lambda: _call(lib, _gp(), b, 2)),
           ("null graph output", lambda: _call(lib, _gp(), b, graph=False)),
           ("null graph output, no msa output", lambda: _call(lib, _gp(), b, out=False, graph=False)),
           ("strand output without reversed", lambda: _call(lib, _gp(), b, strand="no arrays")),
           ("null seq_off", lambda: _call(lib, _gp(), b, 7, seq_off=None)),
           ("null quals beside a quality", lambda: _call(lib, _gp(), b, quals=None)),
           ("a sequence of 65 535 bases", lambda: _call(lib, _gp(), poa.group_batch([["A" * 65535]])))]
    for what, f in bad:
        rc, g = f()
        assert rc == capi.VC_ERR_ARG, what
        assert lib.vc_poa_last_error().decode(), what
        if "null graph output" not in what:                                    # a failed call leaves every pointer NULL
            assert all(not getattr(g, name) for name, _ in capi.VcPoaGraphOut._fields_), what
    # the documented order: vc_poa_run_msa's (scores, then flags), then g, then s, then the batch
    err = lambda: lib.vc_poa_last_error().decode()                         # noqa: E731
    assert _call(lib, _gp(match=500), b, 8, graph=False, strand="no arrays", seq_off=None)[0] == capi.VC_ERR_ARG and "scores" in err()
    assert _call(lib, _gp(), b, 8, graph=False, strand="no arrays", seq_off=None)[0] == capi.VC_ERR_ARG and "flag" in err()
    assert _call(lib, _gp(), b, 1, graph=False, strand="no arrays", seq_off=None)[0] == capi.VC_ERR_ARG and "graph" in err()
    assert _call(lib, _gp(), b, 1, strand="no arrays", seq_off=None)[0] == capi.VC_ERR_ARG and "strand" in err()
    assert _call(lib, _gp(), b, 1, strand="all", seq_off=None)[0] == capi.VC_ERR_ARG and "batch" in err()
    # a call that got as far as the batch has cleared the caller's struct
    g = _call(lib, _gp(), b, 1, seq_off=None)[1]
    assert not g.n_nodes and not g.path_node and g.n_groups == 0


def test_valid_graph_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    for b in (poa.group_batch([["ACGT", ("ACGA", "IIII")], [], ["T"]]), poa.group_batch([])):
        for flags in (0, 1, 3, 4, 7):
            rc, g = _call(lib, _gp(), b, flags)
            assert rc == capi.VC_ERR_NO_DEVICE and not g.n_nodes and not g.cons_node, flags
        assert _call(lib, _gp(), b, out=False)[0] == capi.VC_ERR_NO_DEVICE                    # o == NULL
        assert _call(lib, _gp(), b, 1, strand="all")[0] == capi.VC_ERR_NO_DEVICE              # with spoa's -s
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_graph([["ACGT"]], "semi-global")
    assert ex.value.rc == capi.VC_ERR_NO_DEVICE and "vc_poa_run_graph" in str(ex.value)
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_graph([["ACGT"]], strand_ambiguous=True, msa=True)
    assert "vc_poa_run_graph" in str(ex.value)


# ------------------------------------------------------------------ the formatter on a graph small enough to read
def _tiny():
    """ACGT and AGGT, global: nodes A C G T G', C and G' aligned; the consensus keeps the first read"""
    return G.graph([(b"ACGT", None), (b"AGGT", None)], 1, 5, -4, -8)


def test_formatter_on_a_graph_written_out_by_hand():
    t = _tiny()
    assert t["node_base"] == "ACGTG" and t["aligned"] == [[1, 4]] and t["paths"] == [[0, 0, [0, 1, 2, 3]], [1, 0, [0, 4, 2, 3]]]
    pg = G.to_poa_graph(t)
    assert pg.edges() == [(0, 1, 2), (0, 4, 2), (1, 2, 2), (2, 3, 4), (4, 2, 2)] and pg.aligned_pairs() == [(1, 4)]
    assert pg.paths() == [(0, False, [0, 1, 2, 3]), (1, False, [0, 4, 2, 3])] and pg.n_nodes == 5
    assert t["cons_node"] == [0, 4, 2, 3] and t["consensus"] == "AGGT"      # the tie between C and G' goes to the later node
    assert pg.to_gfa(["x", b"y"], include_consensus=True) == (
        b"H\tVN:Z:1.0\n"
        b"S\t1\tA\tic:Z:true\nL\t1\t+\t2\t+\tOM\tew:f:2\nL\t1\t+\t5\t+\tOM\tew:f:2\tic:Z:true\n"
        b"S\t2\tC\nL\t2\t+\t3\t+\tOM\tew:f:2\n"
        b"S\t3\tG\tic:Z:true\nL\t3\t+\t4\t+\tOM\tew:f:4\tic:Z:true\n"
        b"S\t4\tT\tic:Z:true\n"
        b"S\t5\tG\tic:Z:true\nL\t5\t+\t3\t+\tOM\tew:f:2\tic:Z:true\n"
        b"P\tx\t1+,2+,3+,4+\t*\nP\ty\t1+,5+,3+,4+\t*\nP\tConsensus\t1+,5+,3+,4+\t*\n")
    assert pg.to_gfa(["x", "y"]) == pg.to_gfa(["x", "y"], include_consensus=True).rsplit(b"P\t", 1)[0]
    pg.path_reversed[1] = True                                            # a kept reverse strand: printed backwards, with '-'
    assert b"P\ty\t4-,3-,5-,1-\t*\n" in pg.to_gfa(["x", "y"])
    assert pg.to_dot() == (
        b"digraph 2 {\n  graph [rankdir = LR]\n"
        b'  0[label = "0 - A", style = filled, fillcolor = goldenrod1]\n'
        b'  0 -> 1 [label = "2"]\n  0 -> 4 [label = "2", color = goldenrod1]\n'
        b'  1[label = "1 - C"]\n  1 -> 2 [label = "2"]\n'
        b"  1 -> 4 [style = dotted, arrowhead = none]\n"
        b'  2[label = "2 - G", style = filled, fillcolor = goldenrod1]\n  2 -> 3 [label = "4", color = goldenrod1]\n'
        b'  3[label = "3 - T", style = filled, fillcolor = goldenrod1]\n'
        b'  4[label = "4 - G", style = filled, fillcolor = goldenrod1]\n  4 -> 2 [label = "2", color = goldenrod1]\n}\n')
    # an empty member has no path, and a path is named by its own member (spoa would print the name of record 1 here)
    t = G.graph([(b"ACGT", None), (b"", None), (b"ACGT", None)], 1, 5, -4, -8)
    assert [p[0] for p in t["paths"]] == [0, 2]
    assert b"P\tc\t1+,2+,3+,4+\t*\n" in G.to_poa_graph(t).to_gfa(["a", "b", "c"])
    empty = G.to_poa_graph(G.graph([], 1, 5, -4, -8))
    assert empty.to_gfa([], include_consensus=True) == b"H\tVN:Z:1.0\nP\tConsensus\t\t*\n" and empty.to_dot() == b"digraph 0 {\n  graph [rankdir = LR]\n}\n"


# ------------------------------------------------------------------ the fixture and the restatement
def test_fixture_shape_and_conditions():
    fx = load_graph_fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "poa_graph.json.gz")) <= os.path.getsize(os.path.join(GOLDEN, "poa_strand.json.gz"))
    assert len(fx["kat"]) == 18 and set(fx["kat"]) == set(json.load(open(os.path.join(GOLDEN, "spoa_kat_gaps.json"))))
    assert [g["name"] for g in fx["groups"]] == [g["name"] for g in load_fixture()["groups"]] and len(fx["groups"]) == 30
    assert {g["model"] for g in fx["gaps"]} == {"affine", "convex"} and len(fx["gaps"]) == 10
    strand_fx = json.load(gzip.open(os.path.join(GOLDEN, "poa_strand.json.gz"), "rt"))
    assert all(g["flips"] == s["flips"] for g, s in zip(fx["groups"], strand_fx["groups"]))
    assert all(k["flips"] == strand_fx["kat"][name]["flips"] for name, k in fx["kat"].items())
    assert {g["name"] for g in fx["hand"]} >= {"empty_group", "empty_members_only", "empty_members_between", "single_member", "nodes_63",
                                               "nodes_64", "nodes_65", "members_70_of_20_bases", "out_degree_4_and_aligned_column_of_4",
                                               "weights_from_qualities", "reversed_member_0"}
    es = entries()
    assert len(es) == 2 * (18 + 3 * 30 + 3 * 10 + 3 * len(fx["hand"]))
    by = {l: e for l, *_, e in es}
    with_text = [l for l, *_, e in es if "text" in e]
    assert {l.split("/")[0] for l in with_text if not l.startswith("hand")} == \
        {n for n, k in fx["kat"].items() if k["scores"][2] == k["scores"][3] and not k["quality"]}     # (read 0's quality is all '!')
    assert sum(1 for l in with_text if l.startswith("hand")) >= 30
    full = [G.unpack(e["tables"]) for *_, e in es if "tables" in e]
    assert len(full) >= 100 and all("tables" in e for l, *_, e in es if l.startswith("hand/"))
    for (label, mem, names, t, scores, strand, e), in zip(es):
        assert e["counts"][3] == sum(1 for s, _ in mem if len(s)), label        # a path per non-empty member
        assert e["counts"][4] == sum(len(s) for s, _ in mem), label             # a node per base
        if "tables" not in e:
            continue
        tb = G.unpack(e["tables"])
        assert G.counts(tb) == e["counts"] and G.digest(tb) == e["digest"], label
        N = e["counts"][0]
        assert sorted(tb["rank_to_node"]) == list(range(N)) and len(tb["out_off"]) == N + 1 and tb["out_off"][-1] == e["counts"][1], label
        assert all(a < b for a, b in tb["aligned"]) and tb["aligned"] == sorted(tb["aligned"], key=lambda p: p[0]), label
        assert [m for m, _, _ in tb["paths"]] == [i for i, (s, _) in enumerate(mem) if len(s)], label
        for m, rev, path in tb["paths"]:                                        # every path spells the bytes that were kept
            kept = S.kept_view(mem[m][0], mem[m][1], rev)[0] if strand else mem[m][0]
            assert "".join(tb["node_base"][v] for v in path).encode("latin-1") == kept, (label, m)
            assert strand or not rev, label
        assert "".join(tb["node_base"][v] for v in tb["cons_node"]) == tb["consensus"], label
        assert [tb["node_cons_pos"][v] for v in tb["cons_node"]] == list(range(len(tb["cons_node"]))), label
        assert sum(1 for x in tb["node_cons_pos"] if x >= 0) == len(tb["cons_node"]), label
    # the conditions that keep the fixture from proving nothing
    deg = lambda tb: max((b - a for a, b in zip(tb["out_off"], tb["out_off"][1:])), default=0)      # noqa: E731

    def block(tb):
        n = {}
        for a, _ in tb["aligned"]:
            n[a] = n.get(a, 0) + 1
        return 1 + max(n.values(), default=0)
    assert any(r for tb in full for _, r, _ in tb["paths"]) and any(deg(tb) >= 3 for tb in full) and any(block(tb) >= 3 for tb in full)
    assert any(any(w % 2 for w in tb["edge_weight"]) for tb in full)            # odd weights come from qualities only
    for k in (63, 64, 65):
        assert by[f"hand/nodes_{k}/linear/1/plain"]["counts"][0] == k
    assert by["hand/members_70_of_20_bases/linear/1/plain"]["counts"][3] == 70
    od = G.unpack(by["hand/out_degree_4_and_aligned_column_of_4/linear/1/plain"]["tables"])
    assert deg(od) == 4 and block(od) == 4
    rv = G.unpack(by["hand/reversed_member_0/linear/1/strand"]["tables"])["paths"]
    assert not rv[0][1] and any(r for _, r, _ in rv)
    assert by["hand/empty_group/linear/1/plain"]["counts"] == [0, 0, 0, 0, 0] == by["hand/empty_members_only/linear/1/strand"]["counts"]


def _job(i):
    label, mem, names, t, scores, strand, e = entries()[i]
    check_graph(G.graph(mem, t, *scores, strands=strand), e, names, label)
    return label


def test_restatement_reproduces_every_fixture_entry():
    """the restatement's tables equal spoa's (counts, digest, the tables kept in full), and PoaGraph.to_gfa / to_dot on them are the
    recorded bytes of spoa's own command line"""
    es = entries()
    order = sorted(range(len(es)), key=lambda i: -len(es[i][1]) * sum(len(s) for s, _ in es[i][1]) * (2 if es[i][5] else 1))
    with ProcessPoolExecutor(_workers()) as ex:
        assert len(list(ex.map(_job, order))) == len(es)


# ------------------------------------------------------------------ Python and the command line, with fakes
class _Recorder:
    def __init__(self):
        self.calls = []

    def vc_poa_run_graph(self, p, b, r, o, s, g):
        self.calls.append(({f: getattr(p._obj, f) for f, _ in p._obj._fields_}, o._obj.flags, s is not None))
        return 0

    def vc_poa_last_error(self):
        return b""


def test_python_parameters():
    lib = _Recorder()
    g = [["ACGT", "ACGA", ""], []]
    with pytest.raises((ValueError, TypeError)):                           # a recorder fills nothing: NULL tables do not parse ...
        poa.poa_graph(g, lib=lib)
    with pytest.raises((ValueError, TypeError)):
        poa.poa_graph(g, "local", 3, -5, -4, 0, True, lib, gap_extend=-2, gap_open2=-6, gap_extend2=-1, strand_ambiguous=True, msa=True)
    # ... but the calls were made with the documented parameters
    assert lib.calls[0] == (dict(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8), 0, False)
    assert lib.calls[1] == (dict(device=0, algorithm=0, match=3, mismatch=-5, gap_open=-4, gap_extend=-2, gap_open2=-6, gap_extend2=-1),
                            capi.VC_POA_MSA, True)
    with pytest.raises(TypeError):
        poa.poa_graph(g, "global", 5, -4, -8, 0, True, lib, -6)               # keyword-only
    with pytest.raises(ValueError):
        poa.poa_graph(g, "diagonal", lib=lib)


def test_command_line_graph_options(monkeypatch, tmp_path, capfdbinary):
    a = poa.parse_args(["x.fa"])
    assert (a.gfa, a.gfa_consensus, a.graphviz) == (False, False, None)
    assert poa.parse_args(["--gfa", "x.fa"]).gfa and poa.parse_args(["--gfa-consensus", "-l", "1", "--both-strands", "x.fa"]).gfa_consensus
    a = poa.parse_args(["--graphviz", "out.dot", "--gap-extend", "-6", "-l", "2", "a.fa", "b.fa"])
    assert a.graphviz == "out.dot" and a.files == ["a.fa", "b.fa"] and not a.gfa
    for argv in (["-r", "3", "x.fa"], ["-r", "4", "x.fa"], ["--dot", "o", "x.fa"], ["-d", "o", "x.fa"], ["-s", "x.fa"],
                 ["--strand-ambiguous", "x.fa"], ["--graphviz"]):
        with pytest.raises(SystemExit):
            poa.parse_args(argv)
    capfdbinary.readouterr()
    fa, fb = tmp_path / "x.fa", tmp_path / "y.fa"
    fa.write_text(">r1\nACGT\n>r2\nAGGT\n")
    fb.write_text(">s1\nACGT\n")
    tiny = G.to_poa_graph(_tiny())
    tiny.msa = poa.Msa([b"ACGT", b"AGGT"], [0, 1], b"ACGT", np.array([2, 1, 2, 2], np.uint32))
    got = []

    def fake_graph(batch, params, flags=0, lib=None, strands=False):
        got.append((batch.n_windows, {f: getattr(params, f) for f, _ in params._fields_}, flags, strands))
        return [tiny] * batch.n_windows, np.zeros(batch.n_windows, np.uint8)
    old = []
    monkeypatch.setattr(poa, "run_batch_graph", fake_graph)
    monkeypatch.setattr(poa, "poa_consensus", lambda groups, *a, **k: old.append(("consensus", a, k)) or [b"ACGT"] * len(groups))
    monkeypatch.setattr(poa, "poa_consensus_strands", lambda groups, *a, **k: old.append(("strands", a, k)) or ([b"ACGT"] * len(groups), None))
    monkeypatch.setattr(poa, "poa_msa", lambda groups, *a, **k: old.append(("msa", a, k)) or [tiny.msa] * len(groups))
    # the exclusions: exit status 1 and a message, nothing computed
    for argv in (["--gfa", "-r", "1"], ["--gfa-consensus", "-r", "2"], ["--gfa", "--coverage"], ["--gfa-consensus", "--coverage"]):
        assert poa.main(argv + [str(fa)]) == 1
        assert b"--gfa" in capfdbinary.readouterr().err
    assert not got and not old
    assert poa.main(["--gfa", "-l", "1", str(fa)]) == 0
    assert capfdbinary.readouterr().out == tiny.to_gfa(["r1", "r2"])
    assert got[-1] == (1, dict(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8), 0, False)
    assert poa.main(["--gfa-consensus", "--both-strands", "--gap-extend", "-6", "-g", "-8", str(fa)]) == 0
    assert capfdbinary.readouterr().out == tiny.to_gfa(["r1", "r2"], include_consensus=True)
    assert got[-1][1]["gap_extend"] == -6 and got[-1][2:] == (0, True) and got[-1][1]["algorithm"] == 0
    # --graphviz: FILE, FILE.2, ...; the standard output is the one of the other options
    dot = tmp_path / "g.dot"
    assert poa.main(["--graphviz", str(dot), str(fa), str(fb), str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">Consensus LN:i:4\nAGGT\n" * 3
    assert sorted(p.name for p in tmp_path.glob("g.dot*")) == ["g.dot", "g.dot.2", "g.dot.3"] and dot.read_bytes() == tiny.to_dot()
    assert (tmp_path / "g.dot.3").read_bytes() == tiny.to_dot() and got[-1][0] == 3 and got[-1][2] == 0
    assert poa.main(["--graphviz", str(dot), "-r", "2", str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">r1\nACGT\n>r2\nAGGT\n" and got[-1][2] == capi.VC_POA_MSA | capi.VC_POA_MSA_CONSENSUS
    assert poa.main(["--graphviz", str(dot), "--coverage", "--gfa-consensus", str(fa)]) == 1
    capfdbinary.readouterr()
    assert poa.main(["--graphviz", str(dot), "--coverage", str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">Consensus LN:i:4 CV:B:I,2,1,2,2\nACGT\n" and got[-1][2] == capi.VC_POA_MSA | capi.VC_POA_COVERAGE
    assert not old
    # the existing paths are called as before
    n = len(got)
    assert poa.main(["-l", "1", str(fa)]) == 0 and old[-1] == ("consensus", (1, 5, -4, -8), dict(device=0, gap_extend=None, gap_open2=None, gap_extend2=None))
    assert poa.main(["--both-strands", str(fa)]) == 0 and old[-1] == ("strands", (0, 5, -4, -8), dict(device=0, gap_extend=None, gap_open2=None, gap_extend2=None))
    assert poa.main(["-r", "2", "--gap-extend", "-6", str(fa)]) == 0
    assert old[-1] == ("msa", (0, 5, -4, -8), dict(device=0, include_consensus=True, coverage=False, gap_extend=-6, gap_open2=None, gap_extend2=None))
    assert poa.main(["--coverage", "--both-strands", str(fa)]) == 0 and old[-1][2]["strand_ambiguous"] is True and old[-1][2]["coverage"] is True
    assert len(got) == n
    capfdbinary.readouterr()
    for word in ("--gfa", "--gfa-consensus", "--graphviz", "GFA", "--dot", "--strand-ambiguous", "--both-strands", "poa_graph", "FILE.2"):
        assert word in poa.__doc__, word
    assert "named by its own member" in poa.PoaGraph.to_gfa.__doc__
