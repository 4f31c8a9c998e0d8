"""CPU suite: POA groups that go on from a stored graph (vc_poa_run_from, poa.poa_graph(resumable=True), poa.poa_extend,
poa.poa_align(graphs=...), PoaGraph.save / load) at their boundary, and the argument that the stored state is sufficient:
tests/poa_resume_ref.py rebuilds the restatement's graph from the graph tables plus the aligned lists, at every split point of
every group of tests/golden/poa_groups.json.gz and of every entry of tests/golden/poa_msa.json.gz of at most 8 members, and going
on from there gives the committed consensus and alignment rows (spoa's own bytes) and, node by node, the lists of the one-shot
graph.  One hand-made group shows that the tables without the aligned lists are not enough.

Reading of the issue's case list: every group of poa_groups.json.gz (all of them linear) is split at every k and continued to
its end against the committed consensus; the rows are compared as well wherever poa_msa.json.gz holds the entry and the group
has at most 8 members (the affine and convex entries of that size included)."""
import ctypes as C
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import poa_graph_ref as G
import poa_resume_ref as R
from poa_common import _gp, _workers
from test_poa import _device_visible, load_fixture, members
from test_poa_msa import load_msa_fixture
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR = (5, -4, -8, -8, -8, -8)


# ------------------------------------------------------------------ the boundary
def test_from_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_from" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_from")
    for name, cls in (("vc_poa_state_out", capi.VcPoaStateOut), ("vc_poa_graph_in", capi.VcPoaGraphIn)):
        body = hdr[hdr.index(f"typedef struct {name}"):hdr.index(f"}} {name};")]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(\w+);", body) == [f for f, _ in cls._fields_], name
    assert C.sizeof(capi.VcPoaStateOut) == 24 and C.sizeof(capi.VcPoaGraphIn) == 8 + 15 * 8
    # the header states the id rule, the lifetime, the order of the checks, and why correction has no `from` form
    doc = hdr[hdr.index("Groups that go on from a stored graph"):hdr.index("typedef struct vc_poa_state_out")]
    for word in ("The id rule", "library-owned", "in this order", "vc_poa_run_correct has no `from` form", "VC_ERR_NO_DEVICE only after these"):
        assert word in doc, word
    # nothing existing changed layout
    assert C.sizeof(capi.VcPoaGraphOut) == 19 * 8 and C.sizeof(capi.VcPoaAlignOut) == 80 and C.sizeof(capi.VcPoaMsaOut) == 72


# ------------------------------------------------------------------ the restatement: the state is sufficient
def _cases():
    """-> [(label, members, algorithm, scores, expected consensus, expected rows or None)]"""
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    msa = load_msa_fixture()
    rows = {}
    for g in msa["groups"]:
        m, n, gp = g["scores"]
        for t in ("0", "1", "2"):
            rows[(g["name"], int(t), (m, n, gp, gp, gp, gp))] = g["expected"][t]
    out = []
    for g in load_fixture()["groups"]:
        m, n, gp = g["scores"]
        sc = (m, n, gp, gp, gp, gp)
        for t in ("0", "1", "2"):
            e = g["expected"][t]
            if e["status"] != capi.VC_WIN_OK:
                continue
            x = rows.get((g["name"], int(t), sc)) if len(groups[g["name"]]) <= 8 else None
            out.append((f"{g['name']}/{t}", groups[g["name"]], int(t), sc, e["consensus"].encode("latin-1"), x))
    for g in msa["gaps"]:
        if len(groups[g["name"]]) > 8:
            continue
        for t in ("0", "1", "2"):
            e = g["expected"][t]
            out.append((f"{g['name']}/{g['model']}/{t}", groups[g["name"]], int(t), tuple(g["scores"]), e["consensus"].encode("latin-1"), e))
    return out


def _split_job(case):
    """every split point of one case -> (label, splits checked, what went wrong or None)"""
    label, mem, t, sc, cons, want = case
    gr = R.pm.MsaGraph()
    eng = R.pg.Engine(t, *sc)
    snaps = [(R.state(gr), R.lists(gr))]
    for seq, qual in mem:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
        snaps.append((R.state(gr), R.lists(gr)))
    whole = R.lists(gr)
    for k, (st, li) in enumerate(snaps):
        re_gr = R.rebuild(st)
        if R.lists(re_gr) != li:
            return label, k, f"split {k}: the rebuilt graph's lists differ from the one-shot graph's after {k} members"
        R.build(mem[k:], t, sc, re_gr)
        if R.lists(re_gr) != whole:
            return label, k, f"split {k}: the continued graph's lists differ from the one-shot graph's"
        c, rows, mb, cov = R.outputs(re_gr)
        if c != cons:
            return label, k, f"split {k}: consensus {c!r} is not the committed {cons!r}"
        if want is not None and (rows != [r.encode("latin-1") for r in want["rows"]] or mb[:-1] != want["members"] or cov != want["coverage"]):
            return label, k, f"split {k}: rows, members or coverage are not the committed ones"
    return label, len(snaps), None


def test_rebuilt_graph_continues_as_the_one_shot_graph_at_every_split(built):
    cases = _cases()
    assert len(cases) >= 90 and sum(c[5] is not None for c in cases) >= 40
    with ProcessPoolExecutor(_workers()) as ex:
        res = list(ex.map(_split_job, sorted(cases, key=lambda c: -len(c[1]) ** 2 * max(len(s) for s, _ in c[1] + [(b"", None)]))))
    bad = [(label, why) for label, _, why in res if why]
    assert not bad, bad[:5]
    print(f"[restatement] {len(cases)} cases, {sum(n for _, n, _ in res)} split points: rebuilt from tables + aligned lists and continued, "
          f"the committed consensus and rows and the one-shot graph's lists node by node")


# ------------------------------------------------------------------ the missing table matters
HAND = [(b"TTTT", None), (b"TTATT", None), (b"TTCTT", None), (b"TTGTT", None)]   # a column A / C / G, the G made against the C ...
LATER = [(b"TTTT", None)]                                                       # ... and a member that sorts the graph again


def test_the_export_alone_is_not_enough():
    """Nodes 4 (A), 5 (C), 6 (G) form one aligned class.  The G was made against the C (the alignment's tie rule), so its list is
    [5, 4], which aligned_a / aligned_b (only b > a) cannot tell from [4, 5].  Node 2, the T behind the column, has a smaller id
    than the class, so the next topological sort reaches the class through node 2's in-edges, last tail first: node 6 leads,
    and its list order is the order of ranks 3 and 4."""
    st = R.state(R.build(HAND, 1, LINEAR))
    gs = R.guessed(st)
    assert st["aligned_lists"][4:] == [[5, 6], [4, 6], [5, 4]] and gs["aligned_lists"][4:] == [[5, 6], [4, 6], [4, 5]]
    assert {k for k in st if st[k] != gs[k]} == {"aligned_lists"}            # the export's tables cannot tell them apart
    whole = R.build(HAND + LATER, 1, LINEAR)
    true, guess = R.build(LATER, 1, LINEAR, R.rebuild(st)), R.build(LATER, 1, LINEAR, R.rebuild(gs))
    assert R.lists(true) == R.lists(whole) and R.state(true) == R.state(whole)
    assert G.tables(guess)["rank_to_node"] == [0, 1, 6, 4, 5, 2, 3] != G.tables(whole)["rank_to_node"] == [0, 1, 6, 5, 4, 2, 3]
    assert R.state(guess) != R.state(whole)


# ------------------------------------------------------------------ argument checks before the device
def _three_nodes():
    """AC + AG: nodes A, C, G, edges 0 -> 1 and 0 -> 2, C and G aligned, two paths -> (VcPoaGraphIn, its arrays)"""
    st = R.state(R.build([(b"AC", None), (b"AG", None)], 1, LINEAR))
    assert st["node_base"] == "ACG" and st["aligned_lists"] == [[], [2], [1]] and [p for _, _, p in st["paths"]] == [[0, 1], [0, 2]]
    return poa._graph_in([R.to_poa_graph(st)])


def _from(lib, gin, batch, params=None, graph=True, state=True, qbatch=None, align=True, **override):
    cons, off, status, r, vb = poa._result_buffers(batch)
    for k, v in override.items():
        setattr(vb, k, v)
    g, st = capi.VcPoaGraphOut(), capi.VcPoaStateOut()
    qv = a = None
    if qbatch is not None:
        qv = qbatch.as_struct()
        a = capi.VcPoaAlignOut(flags=1)
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.vc_poa_run_from(C.byref(params or _gp()), ref(gin), C.byref(vb), C.byref(r), None, None, ref(g) if graph else None,
                             ref(st) if state else None, ref(qv), ref(a) if align else None)
    assert not st.al_off and not g.n_nodes                                   # a failed call leaves every pointer NULL
    return rc, lib.vc_poa_last_error().decode()


def test_from_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACT"]])

    def bad(what, word, **change):
        gin, keep = _three_nodes()
        for k, v in change.items():
            if v is None or isinstance(v, int):
                setattr(gin, k, v)
            else:
                keep[k][:len(v)] = v
        rc, msg = _from(lib, gin, b)
        assert rc == capi.VC_ERR_ARG and word in msg, (what, rc, msg)
    # one hand-made bad graph per rule, in the documented order
    bad("two graphs for one group", "one graph per group", n_groups=2)
    bad("null out_off", "null array", out_off=None)
    bad("null n_members", "null array", n_members=None)
    bad("out_off decreases", "decreases", out_off=[0, 2, 1, 2])
    bad("al_off does not start at 0", "start at 0", al_off=[1, 1, 2, 2])
    bad("an empty path", "at least one node", path_off=[0, 2, 2])
    bad("node_off against n_nodes", "prefix sum of n_nodes", node_off=[0, 2])
    bad("null edge_head beside two edges", "null array", edge_head=None)
    bad("edge_head names node 3", "edge_head", edge_head=[1, 3])
    bad("al_node names node 3", "al_node", al_node=[3, 1])
    bad("path_node names node 3", "path_node", path_node=[0, 1, 0, 3])
    bad("rank_to_node names node 3", "rank_to_node", rank_to_node=[0, 1, 3])
    bad("rank_to_node is no permutation", "permutation", rank_to_node=[0, 1, 1])
    bad("an edge runs against the order", "runs against", rank_to_node=[1, 0, 2])
    bad("a node aligned to itself", "its own node", al_node=[1, 1])
    bad("aligned lists not symmetric", "symmetric", al_off=[0, 0, 1, 1])
    bad("a node twice in a list", "twice", al_off=[0, 0, 2, 2], al_node=[2, 2])
    bad("aligned nodes joined by an edge", "joined by an edge", out_off=[0, 1, 2, 2], edge_head=[1, 2])
    bad("a path steps along no edge", "no edge", path_node=[0, 1, 1, 2])
    bad("an edge that no path walks", "lies on no path", path_node=[0, 1, 0, 1])
    bad("a second edge 0 -> 1", "lies on no path", edge_head=[1, 1], path_node=[0, 1, 0, 1])
    bad("path_member beyond n_members", "n_members", path_member=[0, 2])
    # the order: the entry's own pairs of arguments, then the call's arguments and the batch, then `from`, rule by rule
    gin, keep = _three_nodes()
    assert _from(lib, gin, b, qbatch=poa.query_batch([["AC"]]), align=False)[1].startswith("the query batch and the align output")
    assert _from(lib, gin, b, graph=False)[1].startswith("the state output needs")
    keep["edge_head"][1] = 3; keep["path_member"][1] = 9; keep["rank_to_node"][:] = [0, 0, 0]
    rc, msg = _from(lib, gin, b, params=_gp(match=500))
    assert rc == capi.VC_ERR_ARG and "scores" in msg
    rc, msg = _from(lib, gin, b, seq_off=None)
    assert rc == capi.VC_ERR_ARG and "batch" in msg
    rc, msg = _from(lib, gin, b)
    assert rc == capi.VC_ERR_ARG and "edge_head" in msg                      # ids before the order before the members
    keep["edge_head"][1] = 2
    assert "permutation" in _from(lib, gin, b)[1]
    keep["rank_to_node"][:] = [0, 1, 2]
    assert "n_members" in _from(lib, gin, b)[1]


def test_valid_from_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    gin, keep = _three_nodes()
    for batch in (poa.group_batch([["ACT"]]), poa.group_batch([[]])):
        assert _from(lib, gin, batch)[0] == capi.VC_ERR_NO_DEVICE
        assert _from(lib, gin, batch, qbatch=poa.query_batch([["AC", "AG"]]))[0] == capi.VC_ERR_NO_DEVICE
        assert _from(lib, None, batch)[0] == capi.VC_ERR_NO_DEVICE           # from nothing, with the state
        assert _from(lib, gin, batch, graph=False, state=False)[0] == capi.VC_ERR_NO_DEVICE
    empty = poa._graph_in([R.to_poa_graph(R.state(R.build([], 1, LINEAR)))])   # a stored graph without a node
    assert _from(lib, empty[0], poa.group_batch([["ACT"]]))[0] == capi.VC_ERR_NO_DEVICE


# ------------------------------------------------------------------ Python
def test_save_and_load_round_trip(tmp_path):
    sts = [R.state(R.build(m, 1, LINEAR)) for m in (HAND, [], [(b"ACGT", b"IIII"), (b"", None), (b"AGT", None)])]
    graphs = [R.to_poa_graph(st) for st in sts]
    path = str(tmp_path / "graphs.stored")                                   # the name is kept as given
    poa.PoaGraph.save(path, graphs, names=["a.fa", b"b.fa", "c.fa"])
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:                             # numpy arrays only
        assert all(isinstance(z[k], np.ndarray) and z[k].dtype != object for k in z.files)
    back, names = poa.PoaGraph.load(path, names=True)
    assert names == [b"a.fa", b"b.fa", b"c.fa"] and [R.of_poa_graph(g) for g in back] == sts
    assert [g.n_members for g in back] == [4, 0, 3] and all(g.resumable for g in back)
    assert back[0].aligned_lists[4:] == [[5, 6], [4, 6], [5, 4]]
    for g, h in zip(graphs, back):
        for k, dt in poa.PoaGraph._ARRAYS:
            assert getattr(h, k).dtype == dt and np.array_equal(getattr(g, k), getattr(h, k)), k
    assert back[0].to_gfa(["r0", "r1", "r2", "r3"]) == graphs[0].to_gfa(["r0", "r1", "r2", "r3"])
    assert [R.of_poa_graph(g) for g in poa.PoaGraph.load(path)] == sts


def test_a_graph_that_is_not_resumable_is_refused(built, tmp_path):
    plain = G.to_poa_graph(G.tables(R.build(HAND, 1, LINEAR)))               # as poa_graph() returns it without resumable=True
    assert not plain.resumable and plain.aligned_lists is None
    with pytest.raises(ValueError, match="resumable=True"):
        poa.poa_extend([plain], [["TTTT"]])
    with pytest.raises(ValueError, match="resumable=True"):
        poa.poa_align(queries=[["TTTT"]], graphs=[plain])
    with pytest.raises(ValueError, match="resumable"):
        poa.PoaGraph.save(str(tmp_path / "x"), [plain])
    good = R.to_poa_graph(R.state(R.build(HAND, 1, LINEAR)))
    with pytest.raises(ValueError, match="1 graphs for 2 groups"):
        poa.poa_extend([good], [["TTTT"], ["TT"]])


def test_groups_and_graphs_of_poa_align():
    good = R.to_poa_graph(R.state(R.build(HAND, 1, LINEAR)))
    with pytest.raises(ValueError, match="groups to build, or graphs"):
        poa.poa_align(queries=[["TTTT"]])
    with pytest.raises(ValueError, match="needs queries"):
        poa.poa_align(graphs=[good])
    with pytest.raises(ValueError, match="2 query lists for 1 groups"):
        poa.poa_align(queries=[["TTTT"], ["TT"]], graphs=[good])
    with pytest.raises(ValueError, match="1 graphs for 2 groups"):
        poa.poa_align([["TTTT"], ["TT"]], [["TTTT"], ["TT"]], graphs=[good])


def test_command_line_options(capsys):
    a = poa.parse_args(["--save-graphs", "s.npz", "x.fa"])
    assert (a.save_graphs, a.from_graphs, a.files) == ("s.npz", None, ["x.fa"])
    a = poa.parse_args(["--from-graphs", "s.npz", "--align", "q.fa", "--align-out", "o.tsv"])
    assert (a.from_graphs, a.files, a.align) == ("s.npz", [], "q.fa")
    with pytest.raises(SystemExit):
        poa.parse_args([])                                                   # an input file is still required without --from-graphs
    assert "required: FILE" in capsys.readouterr().err
    for extra in (["-r", "1"], ["--coverage"], ["--gfa"], ["--graphviz", "g.dot"], ["--correct", "c.fa"]):
        assert poa.main(["--save-graphs", "s.npz", *extra, "x.fa"]) == 1
        assert "--save-graphs / --from-graphs do not go with" in capsys.readouterr().err
