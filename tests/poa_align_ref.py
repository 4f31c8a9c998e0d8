"""TEST INFRASTRUCTURE: a CPU restatement of spoa's `engine->Align(query, graph, &score)` against the finished graph of a POA
group, the bar for vc_poa_run_align beside the recorded reference (tests/golden/poa_align.json.gz).

The engine and the graph are tests/poa_gaps_ref.py's; Engine.align returns the alignment only, so the score comes from
tests/poa_strand_ref.ScoreEngine, which records the end cell's value where the backtrack is reached and 0 elsewhere (spoa leaves
*score unwritten there).  A query is never added: the graph is built first, by the plain loop, and then only read.
pack / unpack / digest are the fixture's storage of an alignment (first differences; a SHA-256 where the pairs are too many).
"""
import hashlib
import json

import poa_gaps_ref as pg
from poa_strand_ref import ScoreEngine, reverse_complement

OK = 0


def build(members, atype, m, n, g, e=None, q=None, c=None):
    """the plain loop over one group -> (engine, graph)"""
    eng = ScoreEngine(atype, m, n, g, e, q, c)
    gr = pg.Graph()
    for seq, qual in members:
        seq = bytes(seq)
        gr.add_alignment(eng.align(seq, gr), seq, qual)
    return eng, gr


def align_one(eng, gr, query, both_strands=False):
    """-> dict(score, score_rev (None without both_strands), reversed, pairs [[node, pos], ...]) -- main.cpp:287-304 without the add"""
    query = bytes(query)
    aln, s0 = eng.align_score(query, gr)
    if not both_strands:
        return dict(score=s0, score_rev=None, reversed=False, pairs=[list(p) for p in aln])
    aln_r, s1 = eng.align_score(reverse_complement(query), gr)
    rev = not s0 >= s1                                   # ties keep the query as given
    return dict(score=s0, score_rev=s1, reversed=rev, pairs=[list(p) for p in (aln_r if rev else aln)])


def align_queries(members, queries, atype, m, n, g, e=None, q=None, c=None, both_strands=False):
    eng, gr = build(members, atype, m, n, g, e, q, c)
    return [align_one(eng, gr, s, both_strands) for s in queries]


# ------------------------------------------------------------------ the fixture's storage
def _delta(xs):
    return [x - p for x, p in zip(xs, [0] + list(xs[:-1]))]


def _undelta(ds):
    out, acc = [], 0
    for d in ds:
        acc += d
        out.append(acc)
    return out


def digest(pairs):
    return hashlib.sha256(json.dumps([list(map(int, p)) for p in pairs], separators=(",", ":")).encode()).hexdigest()


def pack(r, full):
    """align_one()'s dict -> [score, score_rev, reversed, n, digest or [node deltas, position deltas]]"""
    p = r["pairs"]
    return [r["score"], r["score_rev"], int(r["reversed"]), len(p),
            [_delta([a for a, _ in p]), _delta([b for _, b in p])] if full else digest(p)]


def same(r, packed):
    """does a result (align_one()'s dict, or one made from the device's arrays) equal a packed entry?"""
    score, score_rev, rev, n, body = packed
    if (r["score"], r["score_rev"], int(r["reversed"]), len(r["pairs"])) != (score, score_rev, rev, n):
        return False
    if isinstance(body, str):
        return digest(r["pairs"]) == body
    return [list(map(int, p)) for p in r["pairs"]] == [list(p) for p in zip(_undelta(body[0]), _undelta(body[1]))]


def of_query_alignment(qa):
    """vechat_amd.poa.QueryAlignment -> align_one()'s dict"""
    return dict(score=qa.score, score_rev=qa.score_rev, reversed=qa.reversed, pairs=qa.pairs.tolist())


def path_score(pairs, query, node_base, edges, m, n, g, e):
    """The score of a global alignment recomputed from its pairs alone: match / mismatch per aligned pair, g + (k - 1) e per gap
    run of k -- a run being consecutive pairs with the same side missing -- and nothing else; edges: set of (tail, head), to
    check that consecutive nodes are joined."""
    total, run, prev_node = 0, None, None
    for node, pos in pairs:
        kind = "i" if node == -1 else "d" if pos == -1 else None
        if node != -1:
            assert prev_node is None or (prev_node, node) in edges, (prev_node, node)
            prev_node = node
        if kind is None:
            total += m if query[pos] == node_base[node] else n
            run = None
        else:
            total += e if run == kind else g
            run = kind
    return total
