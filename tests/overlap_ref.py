"""CPU restatement of the overlap rule of include/vechat_hip.h (vc_overlap, vc_overlap_sketch), in plain Python integers.
It shares no code with vechat_amd/csrc/vc_overlap.hip and none with vechat_amd/overlap.py: the windows are enumerated one by
one, the seeds come from a dictionary, the chains from lists.  tests/test_overlap_gpu.py compares the device with it array for
array; tests/test_overlap.py checks it against answers written out by hand and measures its recall."""
import numpy as np

DEFAULTS = dict(k=15, w=5, max_occ=100, max_gap=5000, bandwidth=500, lookback=64, min_chain_score=40, min_anchors=3, min_overlap=500,
                drop_internal=1, same_set=0)
REC = np.dtype([("q_id", "<u4"), ("t_id", "<u4"), ("strand", "u1"), ("q_begin", "<u4"), ("q_end", "<u4"), ("t_begin", "<u4"),
                ("t_end", "<u4"), ("n_anchors", "<u4"), ("score", "<i4"), ("matches", "<u4"), ("block", "<u4")])
TAB = np.dtype([("hash", "<u8"), ("seq", "<u4"), ("pos", "<u4"), ("strand", "u1")])
CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
SKIPPED = "skipped"        # a k-mer equal to its reverse complement: in the window, never its minimum


def mix(x, k):
    m = (1 << (2 * k)) - 1
    x = (~x + (x << 21)) & m
    x ^= x >> 24
    x = (x + (x << 3) + (x << 8)) & m
    x ^= x >> 14
    x = (x + (x << 2) + (x << 4)) & m
    x ^= x >> 28
    x = (x + (x << 31)) & m
    return x


def kmers(seq, k):
    """per position p: None (no k-mer ends here), SKIPPED, or (hash, strand)"""
    out = [None] * len(seq)
    for p in range(k - 1, len(seq)):
        codes = [CODE.get(c) for c in seq[p - k + 1:p + 1]]
        if None in codes:
            continue
        fw = 0
        for c in codes:
            fw = fw * 4 + c
        rv = 0
        for c in reversed(codes):
            rv = rv * 4 + (3 - c)
        out[p] = SKIPPED if fw == rv else (mix(min(fw, rv), k), 1 if rv < fw else 0)
    return out


def sketch_one(seq, k, w):
    """[(pos, hash, strand)] of one sequence"""
    km = kmers(bytes(seq), k)
    chosen = set()
    for s in range(len(km) - w + 1):
        win = km[s:s + w]
        if any(x is None for x in win):
            continue
        real = [(x[0], s + i) for i, x in enumerate(win) if x is not SKIPPED]
        if real:
            chosen.add(min(real)[1])                       # smallest hash, then smallest position
    return [(p, km[p][0], km[p][1]) for p in sorted(chosen)]


def sketch(seqs, k=15, w=5):
    rows = [(h, i, p, st) for i, s in enumerate(seqs) for p, h, st in sketch_one(s, k, w)]
    out = np.zeros(len(rows), TAB)
    for f, col in zip(TAB.names, zip(*rows) if rows else [[]] * 4):
        out[f] = list(col)
    return out


def seeds(targets, queries, k, w, max_occ, same_set):
    """{(t_id, q_id, rel_strand): [(t_pos, q_pos)]}"""
    t_tab = [sketch_one(s, k, w) for s in targets]
    q_tab = t_tab if same_set else [sketch_one(s, k, w) for s in queries]
    q_len = [len(s) for s in (targets if same_set else queries)]
    occ, by_hash = {}, {}
    for tabs in ([t_tab] if same_set else [t_tab, q_tab]):
        for tab in tabs:
            for _, h, _ in tab:
                occ[h] = occ.get(h, 0) + 1
    for qi, tab in enumerate(q_tab):
        for p, h, st in tab:
            by_hash.setdefault(h, []).append((qi, p, st))
    keys = {}
    for ti, tab in enumerate(t_tab):
        for tp, h, tst in tab:
            if occ[h] > max_occ:
                continue
            for qi, qp, qst in by_hash.get(h, ()):
                if same_set and qi == ti:
                    continue
                rel = tst ^ qst
                keys.setdefault((ti, qi, rel), []).append((tp, q_len[qi] - qp + k - 2 if rel else qp))
    return keys


def link(a, b, f_a, P):
    """value of reaching anchor b from anchor a (None: not admissible), and the gain"""
    dt, dq = b[0] - a[0], b[1] - a[1]
    if not (0 < dt <= P["max_gap"] and 0 < dq <= P["max_gap"]):
        return None, 0
    d = abs(dt - dq)
    if d > P["bandwidth"]:
        return None, 0
    gain = min(dt, dq, P["k"])
    cost = 0 if d == 0 else (d * P["k"]) // 100 + (d.bit_length() - 1) // 2
    return f_a + gain - cost, gain


def chain(anchors, P):
    """anchors sorted by (t_pos, q_pos) -> (score, [indices of the chain, first to last], f, pred)"""
    f, pred = [], []
    for i, b in enumerate(anchors):
        best, arg = None, -1
        for j in range(i - 1, max(i - P["lookback"], 0) - 1, -1):          # the largest j first: it keeps a tie
            v, _ = link(anchors[j], b, f[j], P)
            if v is not None and (best is None or v > best):
                best, arg = v, j
        if best is not None and best > P["k"]:
            f.append(best); pred.append(arg)
        else:
            f.append(P["k"]); pred.append(-1)
    end = f.index(max(f))                                                   # the smallest i among the maxima
    path = [end]
    while pred[path[-1]] >= 0:
        path.append(pred[path[-1]])
    return f[end], path[::-1], f, pred


def record(key, anchors, t_len, q_len, P):
    """the record of one key, or None"""
    anchors = sorted(anchors)
    if len(anchors) < P["min_anchors"]:
        return None
    score, path, _, _ = chain(anchors, P)
    if score < P["min_chain_score"] or len(path) < P["min_anchors"]:
        return None
    k = P["k"]
    first, last = anchors[path[0]], anchors[path[-1]]
    matches = k + sum(link(anchors[a], anchors[b], 0, P)[1] for a, b in zip(path, path[1:]))
    t_begin, t_end = first[0] - k + 1, last[0] + 1
    qb, qe = first[1] - k + 1, last[1] + 1
    block = max(qe - qb, t_end - t_begin)
    if block < P["min_overlap"]:
        return None
    if P["drop_internal"]:
        left, right = min(qb, t_begin), min(q_len - qe, t_len - t_end)
        slack = 3 * block // len(path)                     # three mean anchor spacings of this chain, granted to each end
        out_l, out_r = max(left - slack, 0), max(right - slack, 0)
        aligned = block + (left - out_l) + (right - out_r)
        if out_l > 1000 or out_r > 1000 or 5 * aligned < 4 * (aligned + out_l + out_r):
            return None
        t_begin, t_end, qb, qe = t_begin - left, t_end + right, qb - left, qe + right      # out to the nearer read end on both sides
        block = max(qe - qb, t_end - t_begin)
    t_id, q_id, rel = key
    q_begin, q_end = (q_len - qe, q_len - qb) if rel else (qb, qe)
    return (q_id, t_id, rel, q_begin, q_end, t_begin, t_end, len(path), score, matches, block)


def overlaps(targets, queries=None, **params):
    P = dict(DEFAULTS, **params)
    if queries is None:
        P["same_set"] = 1
    qs = targets if P["same_set"] else queries
    keys = seeds(targets, qs, P["k"], P["w"], P["max_occ"], P["same_set"])
    rows = []
    for key, anchors in keys.items():
        r = record(key, anchors, len(targets[key[0]]), len(qs[key[1]]), P)
        if r is not None:
            rows.append(r)
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    out = np.zeros(len(rows), REC)
    for i, r in enumerate(rows):
        out[i] = r
    return out
