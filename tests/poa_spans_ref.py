"""TEST INFRASTRUCTURE: a CPU restatement of span-limited alignment in POA groups, the bar for vc_poa_run_spans beside the fixture
tests/golden/poa_spans.json.gz, which comes from spoa itself.  On top of tests/poa_gaps_ref.py (the engine and the plain graph),
tests/poa_msa_ref.py (the graph with its labels and sequences_), tests/poa_strand_ref.py (the -s choice) and
tests/poa_graph_ref.py (the tables); all are imported, not edited.

  Graph::ExtractSubgraph, Graph::Subgraph          <- vendor/spoa/src/graph.cpp:640-732
  Graph::UpdateAlignment                           <- graph.cpp:734-745
  the loop that uses them                          <- src/window.cpp:195-224, without its rank sort and its 1 % rule: the caller
                                                      says which member has a span

A span is an inclusive pair of node ids; in a group built from nothing the id of base k of sequence 0 is k.  The subgraph keeps
the nodes reached backwards from `end` over in-edges and aligned nodes while the id stays >= begin, numbered in id order, with
their in-edges (AddEdge: weights only) and aligned lists restricted to it, and is sorted topologically on its own.
Nothing here is trusted on its own: tests/test_poa_spans.py requires it to reproduce every fixture entry.
"""
import poa_gaps_ref as pg
import poa_graph_ref as G
import poa_msa_ref as pm
import poa_strand_ref as ps


def subgraph(gr, begin, end):
    """Graph::Subgraph(begin, end, &map) of a pg.Graph -> (the subgraph, a pg.Graph that shares the coder, map: subgraph id -> id)"""
    n = len(gr.code)
    inside = [False] * n
    stack = [end]
    while stack:                                         # ExtractSubgraph(nodes_[end], nodes_[begin])
        c = stack.pop()
        if not inside[c] and c >= begin:
            stack.extend(gr.tail[e] for e in gr.inn[c])
            stack.extend(gr.aligned[c])
            inside[c] = True
    sub = pg.Graph()
    sub.coder, sub.decoder = gr.coder, gr.decoder
    to_sub, to_graph = [None] * n, []
    for v in range(n):
        if inside[v]:
            to_sub[v] = sub.add_node(gr.code[v])
            to_graph.append(v)
    for v in range(n):
        if not inside[v]:
            continue
        for e in gr.inn[v]:
            if to_sub[gr.tail[e]] is not None:
                sub.add_edge(to_sub[gr.tail[e]], to_sub[v], gr.weight[e])
        for a in gr.aligned[v]:
            if to_sub[a] is not None:
                sub.aligned[to_sub[v]].append(to_sub[a])
    sub.toposort()
    return sub, to_graph


def update_alignment(to_graph, aln):
    """Graph::UpdateAlignment"""
    return [(nd if nd == -1 else to_graph[nd], q) for nd, q in aln]


def build(members, spans, atype, m, n, g, e=None, q=None, c=None, strands=False):
    """The flow of vc_poa_run_spans over one group: members = [(sequence bytes, quality bytes or None)], spans = one entry per
    member, None or (begin, end) (member 0's is ignored) -> (the pm.MsaGraph, per member whether the reverse complement was kept,
    forward scores, reverse scores; the last three are None without strands)"""
    gr = pm.MsaGraph()
    eng = ps.ScoreEngine(atype, m, n, g, e, q, c)
    rev, sc, scr = [], [], []
    for k, (seq, qual) in enumerate(members):
        seq = bytes(seq)
        span = spans[k] if spans is not None and k > 0 else None
        target, to_graph = subgraph(gr, *span) if span is not None else (gr, None)
        aln, s0 = eng.align_score(seq, target)
        r = False
        if strands:
            aln_r, s1 = eng.align_score(ps.reverse_complement(seq), target)
            r = not s0 >= s1                             # ties keep the forward strand
            seq, qual = ps.kept_view(seq, qual, r)
            aln = aln_r if r else aln
            rev.append(r); sc.append(s0); scr.append(s1)
        if to_graph is not None:
            aln = update_alignment(to_graph, aln)
        gr.add_alignment(aln, seq, qual)
    return (gr, rev, sc, scr) if strands else (gr, None, None, None)


def run(members, spans, atype, m, n, g, e=None, q=None, c=None, strands=False):
    """-> dict(consensus, rows (the last one the consensus row), members, coverage, tables (poa_graph_ref.tables), reversed)"""
    gr, rev, sc, scr = build(members, spans, atype, m, n, g, e, q, c, strands)
    rows, mem = gr.msa(True)
    cons, cov = gr.summary()
    assert cons == gr.consensus()
    return dict(consensus=cons, rows=rows, members=mem, coverage=cov, tables=G.tables(gr, rev), reversed=rev, score=sc, score_rev=scr)
