"""Scrubbing of chimeric reads on the device, over the C ABI `vc_scrub` (include/vechat_hip.h has the rule): the step the
reference's wrapper leaves to `minimap2 -g | yacrd scrubb` (scripts/vechat:187-201).

  python -m vechat_amd.scrub [-x ava-ont|ava-pb] [-c N] [-n F] [-g MAXGAP] [--min-piece N] [--paf FILE] [--report FILE] [-o OUT] reads

Every overlap of a read with another read is an interval on it; a position that at most -c intervals cover is bad; a read whose
bad positions are more than the fraction -n of it is dropped, every other read is cut into the stretches between its bad regions.
The rule is this library's own, in the spirit of `yacrd -c C -n F scrubb`, not a restatement of it.  Without --paf the overlaps
are this package's own (vechat_amd.overlap on the device, internal matches kept); nothing here computes on the CPU what the device
computes, and without a GPU the call fails."""
import argparse
import ctypes as C
import sys

import numpy as np

from . import capi, seqio
from .capi import VcScrubIn, VcScrubOut, VcScrubParams, _ptr, _take, pack
from .overlap import PRESETS, records_from_paf

CLEAN, BAD_ENDS, CHIMERIC, NOT_COVERED = 0, 1, 2, 3
CLASS_NAMES = ("Clean", "BadEnds", "Chimeric", "NotCovered")
PARAMS = tuple(f for f, _ in VcScrubParams._fields_[1:])
REGION = np.dtype([("read", "<u4"), ("begin", "<u4"), ("end", "<u4")])


def declare(lib):
    """argument types of the scrub entries (a missing symbol is an AttributeError: the library is older than this module)"""
    return capi.bind(lib, ("vc_scrub_default_params", "vc_scrub", "vc_scrub_last_error", "vc_scrub_release"))


def default_params(lib=None, **kw):
    lib = declare(lib or capi.load_hip())
    return capi.params_from_defaults(VcScrubParams, lib.vc_scrub_default_params, PARAMS, "scrub", kw)


def run(lengths, intervals, reads=None, quals=None, device=0, lib=None, **params):
    """One vc_scrub call.  lengths: [n]; intervals: rows (read, begin, end) in any order; reads / quals: [bytes] per read or None.
    Returns a dict of numpy arrays named like the fields of vc_scrub_out (pc_bases / pc_quals as bytes or None) plus the call's
    counters under "stats"."""
    lib = declare(lib or capi.load_hip())
    p = default_params(lib, device=device, **params)
    lens = np.ascontiguousarray(np.asarray(lengths, np.int64).astype(np.uint32))
    iv = np.asarray(intervals, np.int64).reshape(-1, 3) if len(intervals) else np.zeros((0, 3), np.int64)
    if iv.size and (iv.min() < 0 or iv.max() >= 1 << 32):
        raise ValueError("an interval with a negative or a 33-bit number")
    cols = [np.ascontiguousarray(iv[:, i].astype(np.uint32)) for i in range(3)]
    a = VcScrubIn(len(lens), _ptr(lens, C.c_uint32), len(iv), *[_ptr(c, C.c_uint32) for c in cols], None, None, None)
    keep = [lens, cols]
    if reads is not None:
        if len(reads) != len(lens) or (quals is not None and len(quals) != len(lens)):
            raise ValueError("as many reads and qualities as lengths")
        packed, arrays = pack(reads)                         # offsets, and the bases with one pad byte behind them
        a.off, a.bases = packed.off, packed.bases
        keep.append(arrays)
        if quals is not None:
            if any(len(q) != len(s) for q, s in zip(quals, reads)):
                raise ValueError("a quality string of another length than its read")
            packed, arrays = pack(quals)
            a.quals = packed.bases
            keep.append(arrays)
    elif quals is not None:
        raise ValueError("qualities without reads")
    o = VcScrubOut()
    rc = lib.vc_scrub(C.byref(p), C.byref(a), C.byref(o))
    if rc != 0:
        raise RuntimeError(f"vc_scrub failed ({rc}): {lib.vc_scrub_last_error().decode()}")
    n, nr, npc = len(lens), int(o.n_regions), int(o.n_pieces)
    res = dict(reg_read=_take(o.reg_read, nr, np.uint32), reg_begin=_take(o.reg_begin, nr, np.uint32), reg_end=_take(o.reg_end, nr, np.uint32),
               reg_off=_take(o.reg_off, n + 1, np.uint64), klass=_take(o.klass, n, np.uint8), bad_total=_take(o.bad_total, n, np.uint32),
               pc_read=_take(o.pc_read, npc, np.uint32), pc_begin=_take(o.pc_begin, npc, np.uint32), pc_end=_take(o.pc_end, npc, np.uint32),
               pc_off=_take(o.pc_off, npc + 1, np.uint64))
    total = int(res["pc_off"][-1])
    res["pc_bases"] = _take(o.pc_bases, total, np.uint8).tobytes() if o.pc_bases else None
    res["pc_quals"] = _take(o.pc_quals, total, np.uint8).tobytes() if o.pc_quals else None
    res["stats"] = dict(intervals=int(o.n_intervals), events=int(o.n_events), segments=int(o.n_segments), regions=nr, pieces=npc)
    del keep
    return res


def bad_regions(lengths, intervals, coverage=0, max_bad_permille=400, device=0, lib=None):
    """(regions as a record array of REGION ordered by (read, begin), klass [n], bad_total [n])"""
    res = run(lengths, intervals, device=device, lib=lib, coverage=coverage, max_bad_permille=max_bad_permille)
    reg = np.zeros(len(res["reg_read"]), REGION)
    reg["read"], reg["begin"], reg["end"] = res["reg_read"], res["reg_begin"], res["reg_end"]
    return reg, res["klass"], res["bad_total"]


def scrub(reads, intervals, quals=None, coverage=0, max_bad_permille=400, min_piece=1, device=0, lib=None):
    """The pieces of a read set: ([(name_suffix or None, bases, quality or None)], report).  name_suffix is None for a read that
    comes back whole and "_<begin>_<end>" for every other piece; report is the dict of run() -- regions, klass and bad_total per
    read, and pc_read, the read of every piece."""
    res = run([len(s) for s in reads], intervals, reads=reads, quals=quals, device=device, lib=lib, coverage=coverage,
              max_bad_permille=max_bad_permille, min_piece=min_piece)
    out = []
    for i in range(len(res["pc_read"])):
        r, b, e = int(res["pc_read"][i]), int(res["pc_begin"][i]), int(res["pc_end"][i])
        lo, hi = int(res["pc_off"][i]), int(res["pc_off"][i + 1])
        out.append((None if (b == 0 and e == len(reads[r])) else f"_{b}_{e}", res["pc_bases"][lo:hi],
                    res["pc_quals"][lo:hi] if res["pc_quals"] is not None else None))
    return out, res


def intervals_from_records(records, dual):
    """Overlap records (vechat_amd.overlap.RECORD, or anything with q_id, q_begin, q_end, t_id, t_begin, t_end) -> an [m, 3] array of
    (read, begin, end).  dual=True: the query side alone -- the device overlapper's same_set output holds pair (i, j) and pair (j, i)
    both; dual=False: both sides of every record -- a PAF file as minimap2 writes it without --dual=yes."""
    q = np.stack([np.asarray(records[f], np.int64) for f in ("q_id", "q_begin", "q_end")], axis=1).reshape(-1, 3)
    if dual:
        return q
    t = np.stack([np.asarray(records[f], np.int64) for f in ("t_id", "t_begin", "t_end")], axis=1).reshape(-1, 3)
    return np.stack([q, t], axis=1).reshape(-1, 3)


def read_headers(path):
    """the header lines of a FASTA / FASTQ file without their first character, in file order (vechat_amd.seqio keeps the names only)"""
    out = []
    with seqio._open(path) as f:
        while True:
            ln = f.readline()
            if not ln:
                return out
            ln = ln.rstrip(b"\r\n")
            if ln[:1] == b">":
                out.append(ln[1:].decode())
            elif ln[:1] == b"@":
                out.append(ln[1:].decode())
                f.readline(); f.readline(); f.readline()


def format_pieces(pieces, res, names, headers, fastq):
    """the text of scrub()'s pieces: a whole read under its own header line, every other piece as <name>_<begin>_<end>"""
    out = []
    for r, (suffix, bases, qual) in zip(res["pc_read"], pieces):
        head = headers[r] if suffix is None else names[r] + suffix
        if fastq:
            out.append(f"@{head}\n{bases.decode()}\n+\n{qual.decode()}\n")
        else:
            out.append(f">{head}\n{bases.decode()}\n")
    return "".join(out)


def format_report(names, lengths, res):
    """one line per read that is not Clean: <class>\\t<name>\\t<len>\\t<e-b>,<b>,<e>;..."""
    out = []
    for r in np.nonzero(res["klass"] != CLEAN)[0]:
        a, z = int(res["reg_off"][r]), int(res["reg_off"][r + 1])
        regs = ";".join(f"{int(e) - int(b)},{int(b)},{int(e)}" for b, e in zip(res["reg_begin"][a:z], res["reg_end"][a:z]))
        out.append(f"{CLASS_NAMES[int(res['klass'][r])]}\t{names[r]}\t{int(lengths[r])}\t{regs}\n")
    return "".join(out)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vechat_amd.scrub", description="scrub chimeric reads on the MI355X: reads are cut where "
                                 "no other read covers them.  The rule is this library's own, in the spirit of `yacrd -c C -n F scrubb`, "
                                 "not a restatement of it")
    ap.add_argument("-x", dest="preset", default="ava-ont", choices=sorted(PRESETS), help="the overlapper's preset (ava-ont: k 15; ava-pb: k 19)")
    ap.add_argument("-c", dest="coverage", type=int, default=0, help="a position covered by at most N other reads is bad")
    ap.add_argument("-n", dest="not_covered", type=float, default=0.4, help="a read with more than this fraction of bad positions is dropped")
    ap.add_argument("-g", dest="max_gap", type=int, default=5000, help="the overlapper's largest gap between two chained anchors")
    ap.add_argument("--min-piece", type=int, default=1, help="shortest piece kept")
    ap.add_argument("--paf", default=None, help="overlaps from this PAF file (both sides of every record count) instead of the device overlapper")
    ap.add_argument("--report", default=None, help="one line per read that is not clean: class, name, length, its bad regions as length,begin,end;")
    ap.add_argument("-o", dest="out", default="-", help="the scrubbed reads, in the format of the input (default: stdout)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("reads")
    a = ap.parse_args(argv)
    if not 0 <= a.coverage <= 1 << 30:
        ap.error("-c must lie in 0..2^30")
    if not 0.0 <= a.not_covered <= 1.0:
        ap.error("-n must lie in 0..1")
    if a.max_gap <= 0 or a.min_piece < 1:
        ap.error("-g and --min-piece must be positive")
    a.max_bad_permille = int(round(1000 * a.not_covered))
    return a


def main(argv=None, out=None):
    a = parse_args(argv)
    from . import overlap
    recs = seqio.read_sequences(a.reads)
    headers = read_headers(a.reads)
    names, reads = [n for n, _, _ in recs], [d for _, d, _ in recs]
    if len(headers) != len(recs):
        raise ValueError(f"{a.reads}: {len(headers)} header lines for {len(recs)} records")
    with seqio._open(a.reads) as f:
        fastq = f.read(1) == b"@"
    quals = [q if q is not None else b"!" * len(d) for _, d, q in recs] if fastq else None
    if a.paf is None:
        ov = overlap.find_overlaps(reads, None, device=a.device, drop_internal=0, max_gap=a.max_gap, **PRESETS[a.preset])
        intervals = intervals_from_records(ov, dual=True)
    else:
        intervals = intervals_from_records(records_from_paf(a.paf, names, f"is not a read of {a.reads}"), dual=False)
    pieces, res = scrub(reads, intervals, quals=quals, coverage=a.coverage, max_bad_permille=a.max_bad_permille, min_piece=a.min_piece, device=a.device)
    text = format_pieces(pieces, res, names, headers, fastq)
    if out is not None:
        out.write(text)
    elif a.out == "-":
        sys.stdout.write(text)
    else:
        with open(a.out, "w") as fw:
            fw.write(text)
    if a.report:
        with open(a.report, "w") as fw:
            fw.write(format_report(names, [len(d) for d in reads], res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
