"""Hand-built cases of the cluster rule (include/vechat_hip.h, vc_cluster).  A case is a dict: lengths, records -- rows (q_id, t_id,
strand, q_begin, q_end, t_begin, t_end, matches, block) --, params, and `expect`: the answer written out by hand (for the three
large cases: worked out from how the case is built, never by a clusterer) as cl_off, members, cl_root, cl_twisted, cluster, strand,
and the counters links, components, kept.  tests/test_cluster.py runs the restatement (tests/cluster_ref.py) on every case;
tests/test_cluster_gpu.py the device."""
import numpy as np

N = 0xFFFFFFFF                                               # VC_CLUSTER_NONE
FIELDS = ("q_id", "t_id", "strand", "q_begin", "q_end", "t_begin", "t_end", "matches", "block")


def rec(lengths, a, b, strand=0, q=None, t=None, matches=None, block=None):
    """a record of reads a and b: both from end to end, and without an error, unless stated"""
    qb, qe = q or (0, lengths[a])
    tb, te = t or (0, lengths[b])
    block = max(qe - qb, te - tb) if block is None else block
    return (a, b, strand, qb, qe, tb, te, block if matches is None else matches, block)


def case(lengths, records, expect, **params):
    return dict(lengths=list(lengths), records=[tuple(r) for r in records], params=params, expect=expect)


def answer(cl_off, members, cl_root, cl_twisted, cluster, strand, links, components):
    return dict(cl_off=cl_off, members=members, cl_root=cl_root, cl_twisted=cl_twisted, cluster=cluster, strand=strand, links=links,
                components=components, kept=len(cl_root))


def columns(records):
    """rows -> the dict of arrays that vechat_amd.cluster.run takes"""
    a = np.array(records, np.int64).reshape(-1, len(FIELDS))
    return {f: a[:, i] for i, f in enumerate(FIELDS)}


K = [1000] * 8                                               # eight reads of 1 000 bases, for the cases where lengths do not matter
CASES = {
    "no_records": case(K[:3], [], answer([0], [], [], [], [N, N, N], [0, 0, 0], 0, 3)),
    "no_records_every_read_a_cluster_of_one": case(
        K[:3], [], answer([0, 1, 2, 3], [0, 1, 2], [0, 1, 2], [0, 0, 0], [0, 1, 2], [0, 0, 0], 0, 3), min_size=1),
    # a read's record with itself is legal input and links nothing, whatever its strand
    "only_self_records": case(
        K[:2], [rec(K, 0, 0), rec(K, 1, 1, 1), rec(K, 1, 1)], answer([0, 1, 2], [0, 1], [0, 1], [0, 0], [0, 1], [0, 0], 0, 2), min_size=1),
    "one_pair": case(K[:3], [rec(K, 0, 1)], answer([0, 2], [0, 1], [0], [0], [0, 0, N], [0, 0, 0], 1, 2)),
    # single linkage: 0 and 2 share no record
    "chain_of_three_whose_ends_do_not_overlap": case(
        K[:3], [rec(K, 0, 1), rec(K, 2, 1)], answer([0, 3], [0, 1, 2], [0], [0], [0, 0, 0], [0, 0, 0], 2, 1)),
    # 0 - 1 reversed and 1 - 2 reversed: 2 is forward to 0.  Nodes {0, 3, 4} and {1, 2, 5}
    "two_reversals_make_a_forward": case(
        K[:3], [rec(K, 0, 1, 1), rec(K, 1, 2, 1)], answer([0, 3], [0, 1, 2], [0], [0], [0, 0, 0], [0, 1, 0], 2, 1)),
    # + + - around a triangle: no orientation satisfies all three, one component of all six nodes
    "twisted_triangle": case(
        K[:3], [rec(K, 0, 1), rec(K, 1, 2), rec(K, 0, 2, 1)], answer([0, 3], [0, 1, 2], [0], [1], [0, 0, 0], [0, 0, 0], 3, 1)),
    # ... and beside it a pair that is not twisted: the twist belongs to a cluster
    "same_pair_recorded_plus_and_minus": case(
        K[:4], [rec(K, 0, 1), rec(K, 0, 1, 1), rec(K, 2, 3, 1)],
        answer([0, 2, 4], [0, 1, 2, 3], [0, 2], [1, 0], [0, 0, 1, 1], [0, 0, 0, 1], 3, 2)),
    # 3 - 1 reversed, 2 - 3 forward: nodes {3, 4, 6} and {2, 5, 7}; label(2) = 2, label(4) = 3, label(6) = 3
    "root_is_not_read_0": case(
        K[:4], [rec(K, 3, 1, 1), rec(K, 2, 3)], answer([0, 3], [1, 2, 3], [1], [0], [N, 0, 0, 0], [0, 0, 1, 1], 2, 2)),
    # 1000 * 1000 == 800 * 1250 on the query side links 0 - 1; 999 bases do not link 2 - 3
    "cover_on_the_query_side_at_equality_and_one_below": case(
        [1250, 1000, 1250, 1000], [rec(K, 0, 1, q=(250, 1250)), rec(K, 2, 3, q=(250, 1249))],
        answer([0, 2], [0, 1], [0], [0], [0, 0, N, N], [0, 0, 0, 0], 1, 3)),
    "cover_on_the_target_side_at_equality_and_one_below": case(
        [1000, 1250, 1000, 1250], [rec(K, 0, 1, t=(0, 1000)), rec(K, 2, 3, t=(1, 1000))],
        answer([0, 2], [0, 1], [0], [0], [0, 0, N, N], [0, 0, 0, 0], 1, 3)),
    # 1000 * 800 >= 800 * 999 and 1000 * 799 < 800 * 999: the products decide, not a rounded fraction
    "cover_of_a_length_that_800_does_not_divide": case(
        [999, 999, 999, 999], [rec(K, 0, 1, q=(0, 800), t=(0, 999)), rec(K, 2, 3, q=(0, 799), t=(0, 999))],
        answer([0, 2], [0, 1], [0], [0], [0, 0, N, N], [0, 0, 0, 0], 1, 3)),
    # reads of 600: 500 and 499 bases both pass the cover test (480 are asked for), block 499 is below min_overlap
    "min_overlap_at_equality_and_one_below": case(
        [600] * 4, [rec(K, 0, 1, q=(0, 500), t=(100, 600)), rec(K, 2, 3, q=(0, 499), t=(101, 600))],
        answer([0, 2], [0, 1], [0], [0], [0, 0, N, N], [0, 0, 0, 0], 1, 3)),
    # 1000 * 903 >= 900 * 1003 = 902 700 > 1000 * 902
    "identity_at_equality_and_one_below": case(
        [1003] * 6, [rec([1003] * 6, 0, 1, matches=903), rec([1003] * 6, 2, 3, matches=902), rec([1003] * 6, 4, 5, q=(3, 1003), t=(0, 1000), matches=900)],
        answer([0, 2, 4], [0, 1, 4, 5], [0, 4], [0, 0], [0, 0, N, N, 1, 1], [0] * 6, 2, 4), min_identity_permille=900, min_cover_permille=0),
    "identity_0_switches_the_test_off": case(
        K[:2], [rec(K, 0, 1, matches=0)], answer([0, 2], [0, 1], [0], [0], [0, 0], [0, 0], 1, 1)),
    # read 1 lies inside read 0: all of the short read, a third of the long one
    "containment_with_cover_both": case(
        [3000, 1000], [rec(K, 1, 0, q=(0, 1000), t=(500, 1500))], answer([0], [], [], [], [N, N], [0, 0], 0, 2)),
    "containment_with_cover_either": case(
        [3000, 1000], [rec(K, 1, 0, q=(0, 1000), t=(500, 1500))], answer([0, 2], [0, 1], [0], [0], [0, 0], [0, 0], 1, 1), cover_both=0),
    "containment_with_cover_either_from_the_long_read": case(
        [3000, 1000], [rec(K, 0, 1, 1, q=(500, 1500), t=(0, 1000))], answer([0, 2], [0, 1], [0], [0], [0, 0], [0, 1], 1, 1), cover_both=0),
    # a triple, a pair and a single read at min_size 3
    "min_size_drops_a_pair_and_a_singleton": case(
        K[:6], [rec(K, 0, 1), rec(K, 1, 2), rec(K, 3, 4, 1)], answer([0, 3], [0, 1, 2], [0], [0], [0, 0, 0, N, N, N], [0, 0, 0, 0, 1, 0], 3, 3),
        min_size=3),
    "min_size_exactly_met_behind_a_dropped_cluster": case(
        K[:6], [rec(K, 0, 1), rec(K, 2, 3), rec(K, 3, 4), rec(K, 4, 2)], answer([0, 3], [2, 3, 4], [2], [0], [N, N, 0, 0, 0, N], [0] * 6, 4, 3),
        min_size=3),
    # sizes 2, 3, 2: the triple first, then the two pairs by their roots
    "by_size_with_a_tie_in_size": case(
        K[:7], [rec(K, 1, 0), rec(K, 2, 3), rec(K, 4, 3), rec(K, 6, 5)],
        answer([0, 3, 5, 7], [2, 3, 4, 0, 1, 5, 6], [2, 0, 5], [0, 0, 0], [1, 1, 0, 0, 0, 2, 2], [0] * 7, 4, 3), by_size=1),
    "by_size_off_numbers_by_root": case(
        K[:7], [rec(K, 1, 0), rec(K, 2, 3), rec(K, 4, 3), rec(K, 6, 5)],
        answer([0, 2, 5, 7], [0, 1, 2, 3, 4, 5, 6], [0, 2, 5], [0, 0, 0], [0, 0, 1, 1, 1, 2, 2], [0] * 7, 4, 3)),
    # lengths 900, 1000, 1000, 950: the two longest by index, the root stays the smallest index
    "longest_first_with_a_tie_in_length": case(
        [900, 1000, 1000, 950], [rec([900, 1000, 1000, 950], 0, 1), rec([900, 1000, 1000, 950], 1, 2), rec([900, 1000, 1000, 950], 2, 3)],
        answer([0, 4], [1, 2, 3, 0], [0], [0], [0, 0, 0, 0], [0] * 4, 3, 1), longest_first=1),
    "longest_first_and_by_size_together": case(
        [500, 700, 600, 900, 800, 800, 100], [rec([500, 700, 600, 900, 800, 800, 100], a, b) for a, b in ((0, 1), (2, 3), (3, 4), (5, 4))],
        answer([0, 4, 6], [3, 4, 5, 2, 1, 0], [2, 0], [0, 0], [1, 1, 0, 0, 0, 0, N], [0] * 7, 4, 3), by_size=1, longest_first=1, min_overlap=0),
    "duplicated_records_in_both_directions": case(
        K[:2], [rec(K, 0, 1, 1)] * 3 + [rec(K, 1, 0, 1)] * 2, answer([0, 2], [0, 1], [0], [0], [0, 0], [0, 1], 5, 1)),
}


def built(n, pairs, extra_lengths=None):
    """A case from records (a, b, strand) that contradict nothing: every read gets the orientation its records give it, walking
    them in the order given (each record must touch a read that has one, or start a new component), and the answer follows from
    that walk: strand[r] = orientation of r XOR orientation of the smallest read of its component."""
    lengths = extra_lengths or [1000] * n
    orient, comp, nxt = {}, {}, 0
    for a, b, s in pairs:
        if a not in orient and b not in orient:
            orient[a], comp[a] = 0, nxt
            nxt += 1
        if b not in orient:
            orient[b], comp[b] = orient[a] ^ s, comp[a]
        elif a not in orient:
            orient[a], comp[a] = orient[b] ^ s, comp[b]
        else:
            assert comp[a] == comp[b] and orient[a] ^ orient[b] == s
    reads_of = {}
    for r in sorted(comp):
        reads_of.setdefault(comp[r], []).append(r)
    groups = sorted(reads_of.values())                       # by their smallest read
    cluster, strand, members, cl_off = [N] * n, [0] * n, [], [0]
    for c, g in enumerate(groups):
        for r in g:
            cluster[r], strand[r] = c, orient[r] ^ orient[g[0]]
        members += g
        cl_off.append(len(members))
    records = [rec(lengths, a, b, s) for a, b, s in pairs]
    return case(lengths, records, answer(cl_off, members, [g[0] for g in groups], [0] * len(groups), cluster, strand, len(pairs),
                                         len(groups) + n - len(comp)))


def path_pairs(rng, ids):
    """a path through ids in the order given, the records' direction and strand drawn"""
    out = []
    for a, b in zip(ids, ids[1:]):
        out.append((a, b, int(rng.integers(0, 2))) if rng.random() < 0.5 else (b, a, int(rng.integers(0, 2))))
    return out


def star_pairs(rng, hub, leaves):
    return [(hub, x, int(rng.integers(0, 2))) if rng.random() < 0.5 else (x, hub, int(rng.integers(0, 2))) for x in leaves]


def large_cases(seed=5):
    rng = np.random.default_rng(seed)
    # 300 reads on one path whose ids are scrambled along it: 600 nodes over several blocks, deep trees before any jumping
    ids = [int(x) for x in rng.permutation(300)]
    path = path_pairs(rng, ids)
    # a hub with 500 leaves, the hub the largest id: every edge hooks the hub's two nodes, contention on one parent word each
    star = star_pairs(rng, 500, [int(x) for x in rng.permutation(500)])
    # the two side by side, their records interleaved, one read between them that nothing links
    both = path_pairs(rng, [int(x) for x in rng.permutation(300)]) + star_pairs(rng, 801, [int(x) for x in 301 + rng.permutation(500)])
    c = built(802, both)                                     # walked component by component, then the records are mixed
    c["records"] = [c["records"][int(i)] for i in rng.permutation(len(both))]
    return {"path_of_300_reads_with_scrambled_ids": built(300, path), "star_with_a_hub_of_degree_500": built(501, star),
            "path_and_star_side_by_side": c}


CASES.update(large_cases())


def sweep(seed=30, count=36):
    """`count` random record sets over all parameters, from one seed: n up to 2 000 reads, m up to 6 000 records.  The strands follow
    a hidden orientation of the reads, so a cluster is twisted only where a record was flipped on purpose; every third set holds a
    path of 150 reads, so that components deeper than 64 are certain."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(2, 2001)) if i % 4 else int(rng.integers(2, 40))
        m = int(rng.integers(0, min(3 * n, 6000) + 1)) if i else 0              # the first set has reads and no record
        lengths = [int(x) for x in rng.integers(200, 3001, n)]
        orient = rng.integers(0, 2, n)
        flip = (0.0, 0.02, 0.3)[i % 3]
        records = []
        ids = [int(x) for x in rng.permutation(n)[:150]] if i % 3 == 2 and n > 300 else []
        pool = sorted(set(range(n)) - set(ids))                                  # nothing else touches the path: no short cuts
        pairs = [(pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]) for _ in range(m)]
        for r in ids:
            lengths[r] = 2000                                                    # ... and its records pass every threshold of the sweep
        pairs += list(zip(ids, ids[1:]))
        for j, (a, b) in enumerate(pairs):
            s = int(orient[a] ^ orient[b]) ^ int(rng.random() < flip)
            kind = rng.random() if j < m else 0.0                                # the path's records: end to end, without an error
            if kind < 0.6:                                                       # end to end
                q, t = (0, lengths[a]), (0, lengths[b])
            elif kind < 0.8:                                                     # all of a, some of b
                tb = int(rng.integers(0, lengths[b]))
                q, t = (0, lengths[a]), (tb, int(rng.integers(tb + 1, lengths[b] + 1)))
            else:
                qb, tb = int(rng.integers(0, lengths[a])), int(rng.integers(0, lengths[b]))
                q, t = (qb, int(rng.integers(qb + 1, lengths[a] + 1))), (tb, int(rng.integers(tb + 1, lengths[b] + 1)))
            block = max(q[1] - q[0], t[1] - t[0])
            records.append(rec(lengths, a, b, s, q, t, matches=block if kind == 0.0 else int(block * rng.uniform(0.7, 1.0)), block=block))
        if records and rng.random() < 0.5:
            records += [records[int(rng.integers(0, len(records)))] for _ in range(int(rng.integers(1, 20)))]      # duplicates
        out.append(case(lengths, records, None, min_overlap=int(rng.choice([0, 300, 500, 1000])), min_cover_permille=int(rng.choice([0, 500, 800, 1000])),
                        cover_both=int(rng.integers(0, 2)), min_identity_permille=int(rng.choice([0, 800, 950])), min_size=int(rng.choice([1, 2, 3, 10])),
                        by_size=int(rng.integers(0, 2)), longest_first=int(rng.integers(0, 2))))
    return out
