"""TEST INFRASTRUCTURE: a CPU restatement of the haplotype-aware correction of a POA group, the bar for vc_poa_run_correct beside
the recorded reference (tests/golden/poa_correct.json.gz).

The graph and the engines are tests/poa_gaps_ref.py's (the score from tests/poa_strand_ref.ScoreEngine); added here, from the
reference's additions to the vendored spoa (vendor/spoa/src/graph.cpp:811-1179) and the flow of src/window.cpp:283-394:

  prune              Graph::PruneGraph(0, min_confidence, min_support, average_weight): fp64 confidences over the tail's out-edges
                     and the head's in-edges, support against the average weight; 0 / 0 is NaN and fails every comparison
  largest_subgraph   Graph::LargestSubgraph: components by the recursive DFS (live in-edge tails, then live out-edge heads, in
                     list order), the LAST component of the largest size (`>=`), nodes renumbered in its preorder, edges per node
                     in out-list order with weight 0, the coder kept, a topological sort
  add_weights        Graph::AddWeights: consecutive pairs that both have a node and a position add w[q - 1] + w[q] to the edge
                     between them (creating it where there is none); a pair with a -1 breaks the chain
  correct_group      the six steps of include/vechat_hip.h: build, consensus, average weight, prune, rounds, correction

pack / same are the fixture's storage of a group's result.
"""
import hashlib
import math

import poa_gaps_ref as pg
from poa_strand_ref import ScoreEngine


def _div(a, b):
    """a / b as C++ divides doubles"""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a)
    return a / b


def prune(gr, min_conf, min_sup, avg):
    """-> alive flag per edge (min_weight 0)"""
    alive = []
    for e, w in enumerate(gr.weight):
        if w < 0:
            alive.append(False)
            continue
        conf_uv = _div(w, sum(gr.weight[o] for o in gr.out[gr.tail[e]]))
        support = _div(w, avg)
        conf_vu = _div(w, sum(gr.weight[o] for o in gr.inn[gr.head[e]]))
        alive.append(conf_uv >= min_conf and conf_vu >= min_conf and support >= min_sup)
    return alive


def largest_subgraph(gr, alive):
    N = len(gr.code)
    visited = [False] * N
    best = []
    for v0 in range(N):
        if visited[v0]:
            continue
        comp = [v0]
        visited[v0] = True
        stack = [iter([gr.tail[e] for e in gr.inn[v0] if alive[e]] + [gr.head[e] for e in gr.out[v0] if alive[e]])]
        while stack:
            u = next((u for u in stack[-1] if not visited[u]), None)
            if u is None:
                stack.pop()
                continue
            visited[u] = True
            comp.append(u)
            stack.append(iter([gr.tail[e] for e in gr.inn[u] if alive[e]] + [gr.head[e] for e in gr.out[u] if alive[e]]))
        if len(comp) >= len(best):
            best = comp
    sub = pg.Graph()
    sub.coder, sub.decoder = dict(gr.coder), list(gr.decoder)
    new = {v: sub.add_node(gr.code[v]) for v in best}
    for v in best:
        for e in gr.out[v]:
            if alive[e]:
                sub.tail.append(new[v]); sub.head.append(new[gr.head[e]]); sub.weight.append(0)
                sub.out[new[v]].append(len(sub.tail) - 1); sub.inn[new[gr.head[e]]].append(len(sub.tail) - 1)
    sub.toposort()
    return sub


def add_weights(gr, aln, seq, qual):
    if not seq or not aln:
        return
    w = [1] * len(seq) if qual is None else [pg._LUT[b] for b in qual]
    prev = None
    for node, pos in aln:
        if node == -1 or pos == -1:
            prev = None
            continue
        if prev is not None:
            gr.add_edge(prev, node, (w[pos - 1] + w[pos]) & 0xFFFFFFFF)
        prev = node


def base_weight(total, seq, qual):
    """window.cpp:283,295, in double, base by base"""
    if qual is None:
        return total + float(len(seq))
    for b in qual:
        total += 1 - pow(10, (33 - (b - 256 if b >= 128 else b)) / 10.0)
    return total


def correct_group(members, atype, m, n, g, e=None, q=None, c=None, min_confidence=0.22, min_support=0.19, num_prune=3):
    """members [(sequence bytes, quality bytes or None)] -> dict(consensus, reads, scores, stats, pairs, final_nodes); stats counts
    what the flow did: edges pruned, nodes lost to the largest component, edges created by a round's add_weights; pairs: every
    member's final local alignment; final_nodes: the nodes of the final graph"""
    members = [(bytes(s), None if ql is None else bytes(ql)) for s, ql in members]
    eng = ScoreEngine(atype, m, n, g, e, q, c)
    local = ScoreEngine(0, m, n, g, e, q, c)
    gr = pg.Graph()
    total = 0.0
    for seq, qual in members:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
        total = base_weight(total, seq, qual)
    cons = gr.consensus()
    stats = dict(pruned=0, lost=0, created=0)
    first = next(((s, ql) for s, ql in members if s), None)
    if first is None:
        return dict(consensus=cons, reads=[b""] * len(members), scores=[0] * len(members), stats=stats, pairs=[[]] * len(members), final_nodes=0)
    avg = 2.0 * total / len(first[0]) * (1 if first[1] is None else 1000)

    def step(graph):
        alive = prune(graph, min_confidence, min_support, avg)
        sub = largest_subgraph(graph, alive)
        stats["pruned"] += alive.count(False)
        stats["lost"] += len(graph.code) - len(sub.code)
        return sub
    cur = step(gr)
    for _ in range(num_prune - 1):
        for seq, qual in members:
            before = len(cur.tail)
            add_weights(cur, eng.align(seq, cur), seq, qual)
            stats["created"] += len(cur.tail) - before
        cur = step(cur)
    reads, scores, pairs = [], [], []
    for seq, _ in members:
        aln, sc = local.align_score(seq, cur)
        reads.append(bytes(cur.decoder[cur.code[v]] for v, _ in aln if v != -1))
        scores.append(sc)
        pairs.append(aln)
    return dict(consensus=cons, reads=reads, scores=scores, stats=stats, pairs=pairs, final_nodes=len(cur.code))


# ------------------------------------------------------------------ the fixture's storage
def digest(reads):
    return hashlib.sha256(b"\n".join(bytes(r) for r in reads)).hexdigest()


def pack(r, full):
    """correct_group()'s dict -> dict(consensus, scores, lens, reads: the corrections, or their SHA-256 where they are too many)"""
    reads = [bytes(x) for x in r["reads"]]
    return dict(consensus=bytes(r["consensus"]).decode("latin-1"), scores=[int(s) for s in r["scores"]], lens=[len(x) for x in reads],
                reads=[x.decode("latin-1") for x in reads] if full else digest(reads))


def same(r, packed):
    """does a result (consensus, reads, scores) equal a packed entry?  -> "" or what differs"""
    reads = [bytes(x) for x in r["reads"]]
    if bytes(r["consensus"]).decode("latin-1") != packed["consensus"]:
        return "consensus"
    if [int(s) for s in r["scores"]] != packed["scores"]:
        return "scores"
    if [len(x) for x in reads] != packed["lens"]:
        return "lengths"
    if isinstance(packed["reads"], str):
        return "" if digest(reads) == packed["reads"] else "reads (digest)"
    return "" if [x.decode("latin-1") for x in reads] == packed["reads"] else "reads"
