"""CPU restatement of the scrub rule of include/vechat_hip.h (vc_scrub), in plain Python integers.  It shares no code with
vechat_amd/csrc/vc_scrub.hip and none with vechat_amd/scrub.py: the coverage of every position is counted in a list, position by
position, and the regions and pieces are read off that list.  tests/test_scrub_gpu.py compares the device with it array for array;
tests/test_scrub.py checks it against answers written out by hand."""
import numpy as np

DEFAULTS = dict(coverage=0, max_bad_permille=400, min_piece=1)
CLEAN, BAD_ENDS, CHIMERIC, NOT_COVERED = 0, 1, 2, 3
NAMES = {CLEAN: "Clean", BAD_ENDS: "BadEnds", CHIMERIC: "Chimeric", NOT_COVERED: "NotCovered"}


def runs(marks, want):
    """the maximal runs of `want` in a list of booleans, as [b, e)"""
    out, start = [], None
    for p, x in enumerate(marks):
        if x == want and start is None:
            start = p
        if x != want and start is not None:
            out.append((start, p))
            start = None
    if start is not None:
        out.append((start, len(marks)))
    return out


def scrub_read(length, intervals, coverage, max_bad_permille, min_piece):
    """one read: (regions, klass, bad_total, pieces), the intervals as (begin, end)"""
    cov = [0] * length
    for b, e in intervals:
        assert 0 <= b < e <= length
        for p in range(b, e):
            cov[p] += 1
    bad = [c <= coverage for c in cov]
    regions = runs(bad, True)
    bad_total = sum(e - b for b, e in regions)
    if 1000 * bad_total > max_bad_permille * length:
        return regions, NOT_COVERED, bad_total, []
    if any(b > 0 and e < length for b, e in regions):
        klass = CHIMERIC
    else:
        klass = BAD_ENDS if regions else CLEAN
    return regions, klass, bad_total, [(b, e) for b, e in runs(bad, False) if e - b >= min_piece]


def scrub(lengths, intervals, reads=None, quals=None, **params):
    """lengths: [n]; intervals: [(read, begin, end)].  A dict of arrays named and typed like vc_scrub_out: reg_read, reg_begin,
    reg_end, reg_off, klass, bad_total, pc_read, pc_begin, pc_end, pc_off, and pc_bases / pc_quals (bytes, or None when not given)."""
    P = dict(DEFAULTS, **params)
    per_read = [[] for _ in lengths]
    for r, b, e in intervals:
        per_read[r].append((b, e))
    reg, pcs, klass, totals, reg_off = [], [], [], [], [0]
    for r, n in enumerate(lengths):
        regions, k, t, pieces = scrub_read(int(n), per_read[r], P["coverage"], P["max_bad_permille"], P["min_piece"])
        reg += [(r, b, e) for b, e in regions]
        pcs += [(r, b, e) for b, e in pieces]
        klass.append(k); totals.append(t); reg_off.append(len(reg))
    pc_off = [0]
    for _, b, e in pcs:
        pc_off.append(pc_off[-1] + e - b)
    col = lambda rows, i: np.array([x[i] for x in rows], np.uint32)
    return dict(reg_read=col(reg, 0), reg_begin=col(reg, 1), reg_end=col(reg, 2), reg_off=np.array(reg_off, np.uint64),
                klass=np.array(klass, np.uint8), bad_total=np.array(totals, np.uint32),
                pc_read=col(pcs, 0), pc_begin=col(pcs, 1), pc_end=col(pcs, 2), pc_off=np.array(pc_off, np.uint64),
                pc_bases=None if reads is None else b"".join(bytes(reads[r])[b:e] for r, b, e in pcs),
                pc_quals=None if quals is None else b"".join(bytes(quals[r])[b:e] for r, b, e in pcs))


def intervals_of(records, dual):
    """the intervals of overlap records (q_id, q_begin, q_end, t_id, t_begin, t_end): the query side alone when the records hold
    both (i, j) and (j, i), both sides otherwise"""
    out = []
    for q, qb, qe, t, tb, te in records:
        out.append((q, qb, qe))
        if not dual:
            out.append((t, tb, te))
    return out


def format_reads(names, headers, reads, quals, res):
    """the scrubbed FASTA / FASTQ text: a read that is one piece covering all of it keeps its header line, every other piece is
    <name>_<begin>_<end>"""
    out = []
    for i in range(len(res["pc_read"])):
        r, b, e = int(res["pc_read"][i]), int(res["pc_begin"][i]), int(res["pc_end"][i])
        whole = b == 0 and e == len(reads[r])
        head = headers[r] if whole else "%s_%d_%d" % (names[r], b, e)
        if quals is None:
            out.append(">%s\n%s\n" % (head, reads[r][b:e].decode()))
        else:
            out.append("@%s\n%s\n+\n%s\n" % (head, reads[r][b:e].decode(), quals[r][b:e].decode()))
    return "".join(out)


def format_report(names, lengths, res):
    """one line per read that is not Clean: <class>\\t<name>\\t<len>\\t<e-b>,<b>,<e>;..."""
    out = []
    for r, name in enumerate(names):
        if res["klass"][r] == CLEAN:
            continue
        a, z = int(res["reg_off"][r]), int(res["reg_off"][r + 1])
        regs = ";".join("%d,%d,%d" % (int(res["reg_end"][x]) - int(res["reg_begin"][x]), int(res["reg_begin"][x]), int(res["reg_end"][x])) for x in range(a, z))
        out.append("%s\t%s\t%d\t%s\n" % (NAMES[int(res["klass"][r])], name, int(lengths[r]), regs))
    return "".join(out)
