"""CPU restatement of the demultiplexing rule of include/vechat_hip.h (vc_demux): every (read, view, pattern) triple fills its whole
dynamic-programming table, cell by cell as the header writes the recurrence (a row at a time in numpy: the minimum over the cell on
the left is a running minimum of the row), and distance, end and start are read off the tables.  No bit vectors, no column state:
it shares no code path with vechat_amd/csrc/vc_demux.hip and none with vechat_amd/demux.py.  tests/test_demux_gpu.py compares the
device with it array for array; tests/test_demux.py checks it against answers written out by hand."""
import numpy as np

DEFAULTS = dict(window=150, max_err_permille=200, min_margin=2, trim=1, flags=0)
ANY, HEAD, TAIL = 0, 1, 2
NONE, ONE_END, BOTH_ENDS, CONFLICT, AMBIGUOUS = 0, 1, 2, 3, 4
CLASS_NAMES = ("None", "OneEnd", "BothEnds", "Conflict", "Ambiguous")
REQUIRE_BOTH, ORIENT, ALL_HITS = 1, 2, 4
UNASSIGNED = 0xFFFFFFFF
NO_DIST = 255
MAX_LABELS = 1 << 20
IUPAC = dict(A="A", C="C", G="G", T="T", R="AG", Y="CT", S="CG", W="AT", K="GT", M="AC", B="CGT", D="AGT", H="ACT", V="ACG", N="ACGT")
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")            # every other byte is its own complement

MATCH = np.zeros((256, 256), bool)                        # MATCH[pattern byte][read byte]
for _code, _bases in IUPAC.items():
    for _b in _bases:
        MATCH[ord(_code), ord(_b)] = True


def views(read, window):
    """(head, tail): the first L bytes of the read and of its reverse complement, L = min(len, window)"""
    L = min(len(read), window)
    return bytes(read[:L]), bytes(read).translate(COMPLEMENT)[::-1][:L]


def table(pattern, text, anchored):
    """the whole table D[0..m][0..len(text)]: D[i][0] = i; D[0][j] = j when anchored, else 0"""
    m, n = len(pattern), len(text)
    D = np.zeros((m + 1, n + 1), np.int64)
    col = np.arange(n + 1)
    if anchored:
        D[0] = col
    t = np.frombuffer(bytes(text), np.uint8)
    for i in range(1, m + 1):
        mis = (~MATCH[pattern[i - 1]][t]).astype(np.int64)
        row = np.empty(n + 1, np.int64)
        row[0] = i
        row[1:] = np.minimum(D[i - 1][:-1] + mis, D[i - 1][1:] + 1)
        # D[i][j] = min(row[j], D[i][j - 1] + 1) for j = 1, 2, ...: the smallest row[k] + (j - k) over k <= j
        D[i] = np.minimum.accumulate(row - col) + col
    return D


def search(pattern, view):
    """(d, e): the smallest distance of the pattern to a stretch of the view that ends at e, and the smallest such e"""
    last = table(pattern, view, False)[len(pattern)]
    d = int(last.min())
    return d, int(np.nonzero(last == d)[0][0])


def start_of(pattern, view, d, e):
    """s: the shortest stretch view[s:e] at distance d from the pattern"""
    last = table(bytes(pattern)[::-1], bytes(view[:e])[::-1], True)[len(pattern)]
    return e - int(np.nonzero(last == d)[0][0])


def view_result(view, patterns, labels, max_err_permille, min_margin):
    """one view: (pat, dist, start, end, second_dist, state, all (d, e)); state is a label, "none" or "ambig" """
    hits = [search(p, view) for p in patterns]
    accepted = [j for j, (d, _) in enumerate(hits) if 1000 * d <= max_err_permille * len(patterns[j])]
    if not accepted:
        return UNASSIGNED, NO_DIST, 0, 0, NO_DIST, "none", hits
    best = min(accepted, key=lambda j: (hits[j][0], -len(patterns[j]), j))
    d, e = hits[best]
    others = [hits[j][0] for j in accepted if labels[j] != labels[best]]
    second = min(others) if others else NO_DIST
    state = "ambig" if second != NO_DIST and second - d < min_margin else labels[best]
    return best, d, start_of(patterns[best], view, d, e), e, second, state, hits


def classify(head, tail, sides, require_both):
    """(klass, label, flip) of a read from the (pat, state) of its two views"""
    (hp, hs), (tp, ts) = head, tail
    is_label = lambda s: not isinstance(s, str)
    plus = (is_label(hs) and sides[hp] == HEAD) or (is_label(ts) and sides[tp] == TAIL)
    minus = (is_label(hs) and sides[hp] == TAIL) or (is_label(ts) and sides[tp] == HEAD)
    flip = int(minus and not plus)
    if hs == "none" and ts == "none":
        return NONE, UNASSIGNED, flip
    if (plus and minus) or (is_label(hs) and is_label(ts) and hs != ts):
        return CONFLICT, UNASSIGNED, flip
    if is_label(hs) and is_label(ts):
        return BOTH_ENDS, hs, flip
    if (is_label(hs) and ts == "none") or (is_label(ts) and hs == "none"):
        return ONE_END, UNASSIGNED if require_both else (hs if is_label(hs) else ts), flip
    return AMBIGUOUS, UNASSIGNED, flip


def demux(reads, patterns, labels=None, sides=None, quals=None, window=150, max_err_permille=200, min_margin=2, trim=1, flags=0):
    """The whole rule: a dict of arrays named and typed like the fields of vc_demux_out (pc_bases / pc_quals as bytes or None)."""
    n, P = len(reads), len(patterns)
    patterns = [bytes(p) for p in patterns]
    labels = list(range(P)) if labels is None else [int(x) for x in labels]
    sides = [ANY] * P if sides is None else [int(x) for x in sides]
    assert all(1 <= len(p) <= 64 and all(chr(c) in IUPAC for c in p) for p in patterns)
    assert all(0 <= x < MAX_LABELS for x in labels) and all(s in (ANY, HEAD, TAIL) for s in sides) and (P > 0 or n == 0)
    v_pat, v_dist, v_start, v_end, v_second = [], [], [], [], []
    klass, label, flip, begin, end = [], [], [], [], []
    all_dist, all_end, bases, qual_out, piece_off = [], [], [], [], [0]
    for r, read in enumerate(reads):
        read = bytes(read)
        state = []
        for view in views(read, window):
            pat, d, s, e, second, st, hits = view_result(view, patterns, labels, max_err_permille, min_margin)
            v_pat.append(pat); v_dist.append(d); v_start.append(s); v_end.append(e); v_second.append(second)
            state.append((pat, st))
            all_dist += [h[0] for h in hits]
            all_end += [h[1] for h in hits]
        k, lab, f = classify(state[0], state[1], sides, bool(flags & REQUIRE_BOTH))
        klass.append(k); label.append(lab); flip.append(f)
        b, e = 0, len(read)
        if trim and v_pat[2 * r] != UNASSIGNED:
            b = v_end[2 * r] if trim == 1 else v_start[2 * r]
        if trim and v_pat[2 * r + 1] != UNASSIGNED:
            e = len(read) - (v_end[2 * r + 1] if trim == 1 else v_start[2 * r + 1])
        if b >= e:
            e = b
        begin.append(b); end.append(e)
        piece, q = read[b:e], (bytes(quals[r])[b:e] if quals is not None else None)
        if (flags & ORIENT) and f:
            piece, q = piece.translate(COMPLEMENT)[::-1], (q[::-1] if q is not None else None)
        bases.append(piece); qual_out.append(q)
        piece_off.append(piece_off[-1] + e - b)
    n_labels = 1 + max(labels) if P else 0
    groups = [[r for r in range(n) if label[r] == g] for g in range(n_labels)]
    grp_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    u32, u8 = (lambda v: np.array(v, np.uint32)), (lambda v: np.array(v, np.uint8))
    return dict(v_pat=u32(v_pat), v_dist=u8(v_dist), v_start=u32(v_start), v_end=u32(v_end), v_second=u8(v_second),
                klass=u8(klass), label=u32(label), flip=u8(flip), begin=u32(begin), end=u32(end),
                piece_off=np.array(piece_off, np.uint64), pc_bases=b"".join(bases), pc_quals=b"".join(qual_out) if quals is not None else None,
                grp_off=grp_off, grp_reads=u32([r for g in groups for r in g]),
                all_dist=u8(all_dist) if flags & ALL_HITS else None, all_end=u32(all_end) if flags & ALL_HITS else None)


def pieces_of(res):
    """[(bases, quals or None)] per read, from the cut bytes"""
    off = [int(x) for x in res["piece_off"]]
    return [(res["pc_bases"][a:b], res["pc_quals"][a:b] if res["pc_quals"] is not None else None) for a, b in zip(off, off[1:])]


def groups_of(res):
    """the per-label lists of cut (and, with ORIENT, oriented) reads"""
    pcs, off = pieces_of(res), [int(x) for x in res["grp_off"]]
    return [[pcs[int(r)][0] for r in res["grp_reads"][a:b]] for a, b in zip(off, off[1:])]


def format_report(names, label_names, pattern_names, res):
    """one line per read: name, class, label name (* unassigned), flip (+ / -), begin, end, then for head and tail the pattern's
    name (* none), dist, start, end"""
    out = []
    for r, name in enumerate(names):
        lab = int(res["label"][r])
        cols = [name, CLASS_NAMES[int(res["klass"][r])], "*" if lab == UNASSIGNED else label_names[lab], "-" if res["flip"][r] else "+",
                int(res["begin"][r]), int(res["end"][r])]
        for v in (2 * r, 2 * r + 1):
            p = int(res["v_pat"][v])
            cols += ["*", "*", "*", "*"] if p == UNASSIGNED else [pattern_names[p], int(res["v_dist"][v]), int(res["v_start"][v]), int(res["v_end"][v])]
        out.append("\t".join(str(c) for c in cols) + "\n")
    return "".join(out)
