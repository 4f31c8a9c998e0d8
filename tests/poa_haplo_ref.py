"""TEST INFRASTRUCTURE: the haplotype rule of include/vechat_hip.h (vc_poa_run_haplotypes) restated in plain Python on
tests/poa_msa_ref.MsaGraph -- its columns, its Successor walk for the paths, its edge labels -- with a heaviest bundle that takes
the weights and the membership as arguments.  Written from the rule's text, rule by rule, without the kernels: the device is
pinned to this file array for array (tests/test_poa_haplo_gpu.py), and this file to hand answers (tests/poa_haplo_cases.py) and
to spoa's own consensus on the committed fixtures (tests/test_poa_haplo.py).
"""
import poa_gaps_ref as pg
import poa_msa_ref as pm

GAP = -1                                                 # sym: a gap inside a member's span; None: outside of it
HAP_NONE = 0xFF
DEFAULTS = dict(max_haplotypes=2, min_reads=2, min_permille=250, rounds=4, indels=False)


def build(members, atype, m, n, g, e=None, q=None, c=None):
    """the group's graph as vc_poa_run_gaps builds it, and the base weights of every sequence that was added"""
    eng = pg.Engine(atype, m, n, g, e, q, c)
    gr = pm.MsaGraph()
    weights = []
    for seq, qual in members:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
        if len(seq):
            weights.append([1] * len(seq) if qual is None else [pg._LUT[b] for b in qual])
    return gr, weights


def paths(gr):
    out = []
    for s, v in enumerate(gr.sequences):
        p = []
        while v is not None:
            p.append(v)
            v = gr.successor(v, s)
        out.append(p)
    return out


def bundle(gr, weight, nodes, edges):
    """spoa's GenerateConsensus on the graph restricted to `nodes` and `edges` (sets) with weight[e] per edge: rank_to_node order,
    every in-list in its own order, out-degree inside the restriction -> node ids"""
    rank = [v for v in gr.rank if v in nodes]
    if not rank:
        return []
    inn = {v: [e for e in gr.inn[v] if e in edges] for v in rank}
    out = {v: [e for e in gr.out[v] if e in edges] for v in rank}
    scores, pred = {v: -1 for v in range(len(gr.code))}, {v: None for v in range(len(gr.code))}

    def better(it, e):
        tl = gr.tail[e]
        return scores[it] < weight[e] or (scores[it] == weight[e] and pred[it] is not None and scores[pred[it]] <= scores[tl])

    mx = None
    for it in rank:
        for e in inn[it]:
            if better(it, e):
                scores[it], pred[it] = weight[e], gr.tail[e]
        if pred[it] is not None:
            scores[it] += scores[pred[it]]
        if mx is None or scores[mx] < scores[it]:
            mx = it
    pos = {v: r for r, v in enumerate(rank)}
    while out[mx]:                                       # branch completion
        start = mx
        for o in out[start]:
            for e in inn[gr.head[o]]:
                if gr.tail[e] != start:
                    scores[gr.tail[e]] = -1
        mx = None
        for it in rank[pos[start] + 1:]:
            scores[it], pred[it] = -1, None
            for e in inn[it]:
                if scores[gr.tail[e]] == -1:
                    continue
                if better(it, e):
                    scores[it], pred[it] = weight[e], gr.tail[e]
            if pred[it] is not None:
                scores[it] += scores[pred[it]]
            if mx is None or scores[mx] < scores[it]:
                mx = it
    path = [mx]
    while pred[mx] is not None:
        mx = pred[mx]
        path.append(mx)
    path.reverse()
    return path


def _agree(x, y):
    return sum(a * b for a, b in zip(x, y))


def _sign(t):
    return (t > 0) - (t < 0)


def split(gr, max_haplotypes=2, min_reads=2, min_permille=250, rounds=4, indels=False):
    """rules 1 to 7 -> (sites [(column, major, minor, n_major, n_minor)] with alleles as codes or GAP, hap of every label, sizes)"""
    col, C = gr.columns()
    P = paths(gr)
    S = len(P)
    if S == 0:
        return [], [], [0]
    node = [{col[v]: v for v in p} for p in P]
    first = [min(d) for d in node]
    last = [max(d) for d in node]

    def sym(s, c):
        if c in node[s]:
            return gr.code[node[s][c]]
        return GAP if first[s] < c < last[s] else None

    alleles = list(range(len(gr.decoder))) + ([GAP] if indels else [])
    sites = []
    for c in range(C):
        span = sum(first[s] <= c <= last[s] for s in range(S))
        syms = [sym(s, c) for s in range(S)]
        qual = []
        for k, a in enumerate(alleles):
            n = syms.count(a)
            if n >= min_reads and 1000 * n >= min_permille * span:
                qual.append((-n, k, a))
        if len(qual) >= 2:
            qual.sort()
            sites.append((c, qual[0][2], qual[1][2], -qual[0][0], -qual[1][0]))
    M = len(sites)
    v = [[1 if sym(s, c) == a else -1 if sym(s, c) == b else 0 for c, a, b, _, _ in sites] for s in range(S)]
    nz = [sum(x != 0 for x in row) for row in v]
    seeds = [min(range(S), key=lambda s: (-nz[s], s))]
    if nz[seeds[0]] != 0:
        for _ in range(1, max_haplotypes):
            d = [max(_agree(v[s], v[j]) for j in seeds) for s in range(S)]
            s = min(range(S), key=lambda s: (d[s], s))
            if d[s] >= 0:
                break
            seeds.append(s)
    K = len(seeds)
    prof = [list(v[s]) for s in seeds]
    of = [None] * S
    for _ in range(rounds):
        new = [min(range(K), key=lambda k: (-_agree(v[s], prof[k]), k)) for s in range(S)]
        moved, of = new != of, new
        if not moved:
            break
        prof = [[_sign(sum(v[s][m] for s in range(S) if of[s] == k)) for m in range(M)] for k in range(K)]
    size = [of.count(k) for k in range(K)]
    keep = [k for k in range(K) if size[k] >= min_reads]
    if not keep:
        of, keep = [0] * S, [0]
    else:
        of = [of[s] if of[s] in keep else min(keep, key=lambda k: (-_agree(v[s], prof[k]), k)) for s in range(S)]
    order = sorted(keep, key=lambda k: (-of.count(k), min(s for s in range(S) if of[s] == k)))
    ident = {k: i for i, k in enumerate(order)}
    of = [ident[k] for k in of]
    return sites, of, [of.count(i) for i in range(len(order))]


def hap_consensus(gr, weights, of, k):
    """rule 8 -> bytes"""
    P = paths(gr)
    weight, nodes, edges = {}, set(), set()
    for s, p in enumerate(P):
        if of[s] != k:
            continue
        nodes.update(p)
        for i in range(1, len(p)):
            e = next(x for x in gr.out[p[i - 1]] if gr.head[x] == p[i])
            edges.add(e)
            weight[e] = weight.get(e, 0) + ((weights[s][i - 1] + weights[s][i]) & 0xFFFFFFFF)
    return bytes(gr.decoder[gr.code[v]] for v in bundle(gr, weight, nodes, edges))


def haplotypes(members, atype, m, n, g, e=None, q=None, c=None, **rule):
    """one group -> dict(consensus: the group's, haps: [bytes], sizes, members: per member its haplotype or HAP_NONE,
    sites: [(column, major byte, minor byte, n_major, n_minor)] with '-' for a gap)"""
    rule = {**DEFAULTS, **rule}
    gr, weights = build(members, atype, m, n, g, e, q, c)
    sites, of, sizes = split(gr, **rule)
    dec = lambda a: 0x2D if a == GAP else gr.decoder[a]
    mem = [HAP_NONE] * len(members)
    for s, i in enumerate(gr.members):
        mem[i] = of[s]
    return dict(consensus=gr.consensus(), haps=[hap_consensus(gr, weights, of, k) for k in range(len(sizes))], sizes=sizes, members=mem,
                sites=[(c_, dec(a), dec(b), na, nb) for c_, a, b, na, nb in sites])
