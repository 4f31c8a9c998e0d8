"""TEST INFRASTRUCTURE: the two rules of vc_poa_run_assign restated in Python -- the ranking of a query's pairs into a best and
a second group, and the slots of a finished graph's rows (k_lg_slots in vechat_amd/csrc/vc_large_kernels.h) -- over plain lists
and over the graph tables poa_graph returns.  The scores themselves are spoa's: tests/golden/poa_assign.json.gz records them.

Rows: row 0 is the virtual start row that every source reads; row r >= 1 is the node of rank r - 1, and preds[r - 1] lists the
rows (>= 1) it reads.  A source has an empty list and reads row 0.
"""
import heapq

OK, OVERFLOW, INVALID = 0, 2, 4


def rank_pairs(scores, ranked):
    """scores[w], ranked[w] per group in group order -> (best_group, best_score, second_group, second_score): the highest ranked
    score, ties to the lower index (a later group replaces only on strictly greater); second likewise over the other groups;
    -1 / 0 where there is none"""
    bg, bs, sg, ss = -1, 0, -1, 0
    for w, (s, ok) in enumerate(zip(scores, ranked)):
        if not ok:
            continue
        if bg < 0 or s > bs:
            bg, bs, sg, ss = w, s, bg, bs
        elif sg < 0 or s > ss:
            sg, ss = w, s
    return bg, bs, sg, ss


def query_status(pair_status):
    """OVERFLOW if any pair overflowed, else INVALID if any was invalid, else OK"""
    if any(s == OVERFLOW for s in pair_status):
        return OVERFLOW
    return INVALID if any(s != OK for s in pair_status) else OK


def assign(table, pair_status, group_has_node):
    """table[k][w] the kept score of query k against group w, pair_status[k][w] its status, group_has_node[w] -> per query
    (best_group, best_score, second_group, second_score, status)"""
    return [rank_pairs(row, [st == OK and has for st, has in zip(sts, group_has_node)]) + (query_status(sts),)
            for row, sts in zip(table, pair_status)]


def kept(score, score_rev):
    """(the kept strand's score, reversed) of one pair scored on both strands: main.cpp:297, ties keep the query as given"""
    return (score_rev, True) if not score >= score_rev else (score, False)


def last_readers(preds):
    """last[r - 1] for row r: the highest row that reads it, the row itself where none does"""
    last = [r + 1 for r in range(len(preds))]
    for r, ps in enumerate(preds):
        for p in ps:
            last[p - 1] = r + 1
    return last


def slots(preds):
    """-> (slot of every row >= 1, n_slots): the rows upward, each takes the LOWEST free slot (a fresh one when none is free);
    only when a row is complete do the rows it read last, and the row itself when nobody reads it, give theirs back.  Row 0 holds
    slot 0 for good, and n_slots counts it."""
    last, free, slot, n = last_readers(preds), [], [], 1
    for r, ps in enumerate(preds):
        if free:
            s = heapq.heappop(free)
        else:
            s, n = n, n + 1
        slot.append(s)
        for p in sorted(set(ps)):
            if last[p - 1] == r + 1:
                heapq.heappush(free, slot[p - 1])
        if last[r] == r + 1:
            heapq.heappush(free, s)
    return slot, n


def check_slots(preds, slot, n_slots):
    """the invariant: no row shares a slot with row 0, with a row it reads, or with any earlier row that a later row still reads"""
    last = last_readers(preds)
    assert len(slot) == len(preds) and all(1 <= s < n_slots for s in slot), (slot, n_slots)
    for r in range(len(preds)):
        for u in range(r):
            if last[u] >= r + 1:                   # row u + 1 is read by row r + 1 or by a later one
                assert slot[u] != slot[r], (u + 1, r + 1, slot[u])
    assert n_slots == 1 + (max(slot) if slot else 0) or not slot


def rows_of(graph):
    """the predecessor rows of a vechat_amd.poa.PoaGraph in rank order (rows from 1)"""
    rank = {int(v): r for r, v in enumerate(graph.rank_to_node)}
    preds = [[] for _ in rank]
    for v in range(graph.n_nodes):
        for e in range(int(graph.out_off[v]), int(graph.out_off[v + 1])):
            preds[rank[int(graph.edge_head[e])]].append(rank[v] + 1)
    return preds


# Hand-built graphs as predecessor lists, with the n_slots the rule gives (worked out by hand in tests/test_poa_assign.py) ...
HAND_ROWS = {
    "chain": ([[]] + [[r] for r in range(1, 5)], 3),
    "one_bubble": ([[], [1], [1], [2, 3]], 4),
    "skip_edge_first_to_last": ([[], [1], [2], [3], [4], [5, 1]], 4),
    "in_degree_9": ([[]] + [[1]] * 9 + [list(range(2, 11))], 11),
    "wide_20_chains": ([[]] * 20 + [[r - 20] for r in range(21, 61)], 22),
    "one_node": ([[]], 2),
}

# ... and as groups whose graphs have those shapes under global alignment with 5 / -4 / -8 (bytes outside ACGT are plain
# symbols to spoa): the members of "wide" share no byte, so every column holds 20 aligned nodes and no two members share a node
_MID = b"CGGCCGCGGCCGGCGCCGCG"
HAND_GROUPS = {
    "chain": [b"ACGTACGTAC", b"ACGTACGTAC"],
    "one_bubble": [b"ACGTACGTAC", b"ACGTTCGTAC"],
    "skip_edge_first_to_last": [b"A" + _MID + b"T", b"AT"],
    "in_degree_9": [b"GG" + bytes([c]) + b"ACGTACGT" for c in b"BDEFHIJKL"],
    "wide_20_chains": [bytes([65 + k]) * 8 for k in range(20)],
    "one_node": [b"A"],
}
