"""TEST INFRASTRUCTURE: a POA group that goes on from a stored graph, restated on the CPU -- the bar for vc_poa_run_from.

  state(gr)      what a call hands out of a finished pm.MsaGraph: the tables of tests/poa_graph_ref.py (vc_poa_graph_out) plus
                 every node's aligned list in list order (vc_poa_state_out) and the number of members so far
  rebuild(st)    the restatement's graph object from those alone, as include/vechat_hip.h argues it can be done: node ids and
                 codes; out-lists in the edge order of out_off; aligned lists as stored; in-lists and labels by replaying the
                 paths in sequences_ order (an edge's first label is the sequence that created it, and a sequence creates at most
                 one edge into a head); coder / decoder by first appearance over the bytes the paths spell, in order
  lists(gr)      the rebuilt graph and the one-shot graph, node by node, in a form that does not depend on edge ids
  guessed(st)    the state with the aligned lists guessed from the export's pairs alone (ascending ids): what is NOT enough

On top of tests/poa_gaps_ref.py (the engine), tests/poa_msa_ref.py (the graph with labels and sequences_) and
tests/poa_graph_ref.py (the tables); all imported, none edited.  tests/test_poa_resume.py requires rebuild + continue to
reproduce the committed consensus and alignment rows, which are spoa's own bytes, at every split point.
"""
import poa_gaps_ref as pg
import poa_graph_ref as G
import poa_msa_ref as pm


def state(gr, reversed_=None):
    """a pm.MsaGraph after its last add_alignment -> dict: G.tables() + aligned_lists + n_members"""
    t = G.tables(gr, reversed_)
    t["aligned_lists"] = [list(a) for a in gr.aligned]
    t["n_members"] = gr._calls
    return t


def guessed(st):
    """the state without vc_poa_state_out: the aligned lists guessed from the pairs (a < b) of the export, ascending"""
    t = dict(st)
    al = [[] for _ in st["node_base"]]
    for a, b in st["aligned"]:
        al[a].append(b)
        al[b].append(a)
    t["aligned_lists"] = [sorted(x) for x in al]
    return t


def rebuild(st):
    """the state -> a pm.MsaGraph that continues as the graph it was taken from does"""
    gr = pm.MsaGraph()
    base = st["node_base"].encode("latin-1")
    for _, _, path in st["paths"]:                          # coder / decoder: first appearance over the kept bytes, in order
        for v in path:
            if base[v] not in gr.coder:
                gr.coder[base[v]] = len(gr.decoder)
                gr.decoder.append(base[v])
    for v, b in enumerate(base):
        gr.add_node(gr.coder[b])
        gr.aligned[v] = list(st["aligned_lists"][v])
    off = st["out_off"]
    for v in range(len(base)):                              # edge id = CSR index: ids are not observable, the list orders are
        for k in range(off[v], off[v + 1]):
            gr.tail.append(v); gr.head.append(st["edge_head"][k]); gr.weight.append(st["edge_weight"][k])
            gr.labels.append([])
            gr.out[v].append(k)
    for k, (member, _, path) in enumerate(st["paths"]):
        for u, v in zip(path, path[1:]):
            e = next(x for x in gr.out[u] if gr.head[x] == v)
            if not gr.labels[e]:
                gr.inn[v].append(e)                         # this sequence created the edge
            gr.labels[e].append(k)
        gr.sequences.append(path[0])
        gr.members.append(member)
    gr._calls = st["n_members"]
    gr.rank = list(st["rank_to_node"])
    return gr


def lists(gr):
    """a graph as what later steps can observe of it: per node its byte, out-list, in-list and aligned list, the edges by their
    ends, weights and labels; then rank, sequences_, members, decoder and the call count"""
    edge = lambda e: (gr.tail[e], gr.head[e], gr.weight[e], tuple(gr.labels[e]))
    return dict(nodes=[(gr.decoder[c], [edge(e) for e in gr.out[v]], [edge(e) for e in gr.inn[v]], list(gr.aligned[v]))
                       for v, c in enumerate(gr.code)],
                rank=list(gr.rank), sequences=list(gr.sequences), members=list(gr.members), decoder=list(gr.decoder),
                coder=dict(gr.coder), calls=gr._calls)


def build(members, atype, scores, start=None):
    """spoa's flow over members = [(sequence, quality or None)] with the engine of scores = (m, n, g, e, q, c), from nothing or
    from the graph `start` -> the graph"""
    eng = pg.Engine(atype, *scores)
    gr = pm.MsaGraph() if start is None else start
    for seq, qual in members:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
    return gr


def outputs(gr):
    """-> (consensus, rows with the consensus row, members, coverage) of a finished graph"""
    rows, mem = gr.msa(True)
    cons, cov = gr.summary()
    return cons, rows, mem, cov


# ------------------------------------------------------------------ between the restatement's dict and vechat_amd.poa.PoaGraph
def of_poa_graph(g):
    """a resumable vechat_amd.poa.PoaGraph -> the dict of state()"""
    t = G.of_poa_graph(g)
    t["aligned_lists"] = g.aligned_lists
    t["n_members"] = g.n_members
    return t


def to_poa_graph(st):
    """the dict of state() -> a resumable vechat_amd.poa.PoaGraph"""
    import numpy as np
    g = G.to_poa_graph(st)
    off = [0]
    for a in st["aligned_lists"]:
        off.append(off[-1] + len(a))
    g.al_off, g.al_node = np.array(off, np.int64), np.array([x for a in st["aligned_lists"] for x in a], np.uint32)
    g.n_members = st["n_members"]
    return g
