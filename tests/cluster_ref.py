"""The clusterer's rule (include/vechat_hip.h, vc_cluster) restated in plain Python, record by record and node by node: an adjacency
list over the 2 n nodes and a breadth-first search from every node in ascending order, so the first node that reaches a component
is its smallest.  It shares no code with vechat_amd/csrc/vc_cluster.hip (union by atomicMin, radix sorts, scans) or with
vechat_amd/cluster.py; tests/test_cluster_gpu.py compares the device with it array for array."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
DEFAULTS = dict(min_overlap=500, min_cover_permille=800, cover_both=1, min_identity_permille=0, min_size=2, by_size=0, longest_first=0)
FIELDS = ("q_id", "t_id", "strand", "q_begin", "q_end", "t_begin", "t_end", "matches", "block")


def links(lengths, rec, P):
    """does the record link its two reads?"""
    a, b, _, qb, qe, tb, te, matches, block = rec
    if a == b or block < P["min_overlap"]:
        return False
    if P["min_identity_permille"] and 1000 * matches < P["min_identity_permille"] * block:
        return False
    ca = 1000 * (qe - qb) >= P["min_cover_permille"] * lengths[a]
    cb = 1000 * (te - tb) >= P["min_cover_permille"] * lengths[b]
    return (ca and cb) if P["cover_both"] else (ca or cb)


def labels(n, edges):
    """label[v] = the smallest node of v's component, by breadth-first search; (labels, the depth of the deepest search)"""
    adj = [[] for _ in range(2 * n)]
    for u, v in edges:
        adj[u].append(v)
        adj[v].append(u)
    label, deepest = [-1] * (2 * n), 0
    for s in range(2 * n):
        if label[s] >= 0:
            continue
        label[s] = s
        todo = deque([(s, 0)])
        while todo:
            u, d = todo.popleft()
            deepest = max(deepest, d)
            for v in adj[u]:
                if label[v] < 0:
                    label[v] = s
                    todo.append((v, d + 1))
    return label, deepest


def cluster(lengths, records, **params):
    """records: rows (q_id, t_id, strand, q_begin, q_end, t_begin, t_end, matches, block).  The dict of vechat_amd.cluster.run()
    without "rounds" among its stats, and "depth": the deepest breadth-first search, for the tests that ask for deep components."""
    P = dict(DEFAULTS, **params)
    lengths = [int(x) for x in lengths]
    n = len(lengths)
    edges, n_links = [], 0
    for rec in records:
        rec = tuple(int(x) for x in rec)
        if links(lengths, rec, P):
            a, b, s = rec[:3]
            edges += [(2 * a, 2 * b + s), (2 * a + 1, 2 * b + 1 - s)]
            n_links += 1
    label, depth = labels(n, edges)
    root = [label[2 * r] >> 1 for r in range(n)]
    strand = [label[2 * r] & 1 for r in range(n)]
    twisted = [int(label[2 * r] == label[2 * r + 1]) for r in range(n)]
    by_root = {}
    for r in range(n):
        by_root.setdefault(root[r], []).append(r)
    kept = [x for x in sorted(by_root) if len(by_root[x]) >= P["min_size"]]
    if P["by_size"]:
        kept.sort(key=lambda x: (-len(by_root[x]), x))
    cl_off, members, cluster_of = [0], [], [NONE] * n
    for c, x in enumerate(kept):
        rows = sorted(by_root[x], key=(lambda r: (-lengths[r], r)) if P["longest_first"] else None)
        for r in rows:
            cluster_of[r] = c
        members += rows
        cl_off.append(len(members))
    return dict(cl_off=np.array(cl_off, np.uint64), members=np.array(members, np.uint32), cl_root=np.array(kept, np.uint32),
                cl_twisted=np.array([twisted[x] for x in kept], np.uint8), cluster=np.array(cluster_of, np.uint32),
                strand=np.array(strand, np.uint8),
                stats=dict(records=len(records), links=n_links, components=len(by_root), kept=len(kept)), depth=depth)


def rows_of(records):
    """a structured array or a dict of arrays with FIELDS -> rows"""
    return [tuple(int(records[f][i]) for f in FIELDS) for i in range(len(records[FIELDS[0]]))]


_COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97}


def groups_of(res, reads):
    out = []
    for c in range(len(res["cl_off"]) - 1):
        g = []
        for r in res["members"][int(res["cl_off"][c]):int(res["cl_off"][c + 1])]:
            s = reads[int(r)]
            g.append(bytes(_COMPLEMENT.get(x, x) for x in reversed(s)) if res["strand"][int(r)] else bytes(s))
        out.append(g)
    return out


def format_tsv(names, res):
    lines = []
    for r, name in enumerate(names):
        c = int(res["cluster"][r])
        where = "*" if c == NONE else str(c)
        strand = "?" if c != NONE and res["cl_twisted"][c] else "+-"[int(res["strand"][r])]
        lines.append(name + "\t" + where + "\t" + strand + "\n")
    return "".join(lines)
