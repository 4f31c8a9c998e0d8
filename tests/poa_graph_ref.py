"""TEST INFRASTRUCTURE: a CPU restatement of the partial order graph as spoa's command line prints it, the bar for
vc_poa_run_graph beside the fixture tests/golden/poa_graph.json.gz, which comes from spoa itself.  On top of
tests/poa_msa_ref.py (the graph with its labels and sequences_) and tests/poa_strand_ref.py (the -s loop); both are imported,
not edited.

  the tables: nodes, out-edges, aligned nodes            <- the order PrintGfa / PrintDot walk them in,
                                                            vendor/spoa/src/main.cpp:139-164, src/graph.cpp:764-800
  a path: sequences_[i], then Node::Successor(i)          <- main.cpp:166-176, graph.cpp:25-39
  the consensus path                                      <- Graph::consensus(), TraverseHeaviestBundle

Everything is the reference's literal walk: a path follows Successor node by node, the edges are read out-list by out-list.
Nothing here is trusted on its own: tests/test_poa_graph.py requires it to reproduce every fixture entry.
"""
import hashlib
import json

import poa_gaps_ref as pg
import poa_msa_ref as pm
import poa_strand_ref as ps


def tables(gr, reversed_=None):
    """the graph of a pm.MsaGraph after its last add_alignment -> dict of plain lists, node ids as spoa's (creation order)
    reversed_: per call of add_alignment (empty members included) whether the reverse complement was kept, or None"""
    cons = gr.consensus_path()
    pos = [-1] * len(gr.code)
    for k, v in enumerate(cons):
        pos[v] = k
    out_off, head, weight = [0], [], []
    for v in range(len(gr.code)):
        for e in gr.out[v]:
            head.append(gr.head[e])
            weight.append(gr.weight[e])
        out_off.append(len(head))
    aligned = [[a, b] for a in range(len(gr.code)) for b in gr.aligned[a] if b > a]
    paths = []
    for i, begin in enumerate(gr.sequences):
        path, it = [], begin
        while it is not None:
            path.append(it)
            it = gr.successor(it, i)
        paths.append([gr.members[i], int(bool(reversed_[gr.members[i]])) if reversed_ is not None else 0, path])
    return dict(node_base=bytes(gr.decoder[c] for c in gr.code).decode("latin-1"), node_cons_pos=pos, rank_to_node=list(gr.rank),
                out_off=out_off, edge_head=head, edge_weight=weight, aligned=aligned, paths=paths, cons_node=cons,
                consensus=bytes(gr.decoder[gr.code[v]] for v in cons).decode("latin-1"))


def graph(members, atype, m, n, g, e=None, q=None, c=None, strands=False):
    """spoa's flow over one group (with -s when strands): members = [(sequence bytes, quality bytes or None)] -> tables()"""
    gr = pm.MsaGraph()
    if not strands:
        eng = pg.Engine(atype, m, n, g, e, q, c)
        for seq, qual in members:
            gr.add_alignment(eng.align(seq, gr), seq, qual)
        return tables(gr)
    eng = ps.ScoreEngine(atype, m, n, g, e, q, c)
    rev = []
    for seq, qual in members:
        seq = bytes(seq)
        aln, s0 = eng.align_score(seq, gr)
        aln_r, s1 = eng.align_score(ps.reverse_complement(seq), gr)
        r = not s0 >= s1
        ks, kq = ps.kept_view(seq, qual, r)
        gr.add_alignment(aln_r if r else aln, ks, kq)
        rev.append(r)
    return tables(gr, rev)


def of_poa_graph(g):
    """a vechat_amd.poa.PoaGraph -> the same dict, for comparison"""
    return dict(node_base=g.node_base.tobytes().decode("latin-1"), node_cons_pos=g.node_cons_pos.tolist(),
                rank_to_node=g.rank_to_node.tolist(), out_off=g.out_off.tolist(), edge_head=g.edge_head.tolist(),
                edge_weight=g.edge_weight.tolist(), aligned=[list(p) for p in g.aligned_pairs()],
                paths=[[m, int(r), p] for m, r, p in g.paths()], cons_node=g.cons_node.tolist(), consensus=g.consensus.decode("latin-1"))


def to_poa_graph(t):
    """the dict -> a vechat_amd.poa.PoaGraph (the formatter under test runs on fixture arrays too)"""
    import numpy as np

    from vechat_amd import poa
    off = [0]
    for _, _, p in t["paths"]:
        off.append(off[-1] + len(p))
    return poa.PoaGraph(node_base=np.frombuffer(t["node_base"].encode("latin-1"), np.uint8), node_cons_pos=np.array(t["node_cons_pos"], np.int32),
                        rank_to_node=np.array(t["rank_to_node"], np.uint32), out_off=np.array(t["out_off"], np.int64),
                        edge_head=np.array(t["edge_head"], np.uint32), edge_weight=np.array(t["edge_weight"], np.int64),
                        aligned_a=np.array([a for a, _ in t["aligned"]], np.uint32), aligned_b=np.array([b for _, b in t["aligned"]], np.uint32),
                        path_member=np.array([m for m, _, _ in t["paths"]], np.uint32), path_reversed=np.array([bool(r) for _, r, _ in t["paths"]], bool),
                        path_off=np.array(off, np.int64), path_node=np.array([v for _, _, p in t["paths"] for v in p], np.uint32),
                        cons_node=np.array(t["cons_node"], np.uint32), consensus=t["consensus"].encode("latin-1"))


# ------------------------------------------------------------------ the fixture's number lists: first differences, which gzip well
_LISTS = ("node_cons_pos", "rank_to_node", "out_off", "edge_head", "edge_weight", "cons_node")


def _delta(xs):
    return [x - p for x, p in zip(xs, [0] + list(xs[:-1]))]


def _undelta(ds):
    out, acc = [], 0
    for d in ds:
        acc += d
        out.append(acc)
    return out


def pack(t):
    """tables() -> the form kept in tests/golden/poa_graph.json.gz"""
    p = dict(t)
    for k in _LISTS:
        p[k] = _delta(t[k])
    p["aligned"] = [_delta([a for a, _ in t["aligned"]]), _delta([b for _, b in t["aligned"]])]
    p["paths"] = [[m, r, _delta(nodes)] for m, r, nodes in t["paths"]]
    return p


def unpack(p):
    t = dict(p)
    for k in _LISTS:
        t[k] = _undelta(p[k])
    t["aligned"] = [[a, b] for a, b in zip(_undelta(p["aligned"][0]), _undelta(p["aligned"][1]))]
    t["paths"] = [[m, r, _undelta(d)] for m, r, d in p["paths"]]
    return t


def digest(t):
    """SHA-256 of the tables in a canonical form: what the fixture keeps of a graph too large to be kept in full"""
    return hashlib.sha256(json.dumps(t, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def counts(t):
    """[nodes, edges, aligned pairs, paths, path entries]"""
    return [len(t["node_base"]), len(t["edge_head"]), len(t["aligned"]), len(t["paths"]), sum(len(p) for _, _, p in t["paths"])]
