"""Demultiplexing, orienting and trimming of reads by adapter, primer and barcode on the device, over the C ABI `vc_demux`
(include/vechat_hip.h has the rule): the step in front of the POA groups that otherwise goes to cutadapt, porechop or minibar.

  python -m vechat_amd.demux [-w WINDOW] [-e MAX_ERR] [--min-margin N] [--trim 0|1|2] [--both-ends] [--orient]
                             [--report FILE.tsv] [--out-dir DIR | -o FILE] [--unassigned FILE]
                             [--consensus FILE [-l 0|1|2]] [--device D] patterns.fa reads

Every pattern (barcode, primer, adapter; IUPAC codes allowed) is searched with errors in the first WINDOW bases of every read and of
its reverse complement; the best pattern at each end gives the read its label, its strand and the range that is kept.  The rule is
this library's own, in the spirit of cutadapt and minibar and a restatement of neither: no adapters beyond the windows, unit
costs, no quality trimming.  Nothing here computes on the CPU what the device computes, and without a GPU the call fails."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import capi, seqio
from .capi import VcDemuxIn, VcDemuxOut, VcDemuxParams, _ptr, _take, pack
from .overlap import COMPLEMENT

ANY, HEAD, TAIL = 0, 1, 2
NONE, ONE_END, BOTH_ENDS, CONFLICT, AMBIGUOUS = 0, 1, 2, 3, 4
CLASS_NAMES = ("None", "OneEnd", "BothEnds", "Conflict", "Ambiguous")
REQUIRE_BOTH, ORIENT, ALL_HITS = 1, 2, 4
UNASSIGNED = 0xFFFFFFFF
SIDES = dict(any=ANY, head=HEAD, tail=TAIL)
PARAMS = tuple(f for f, _ in VcDemuxParams._fields_[1:])
ARRAYS = ("v_pat", "v_dist", "v_start", "v_end", "v_second", "klass", "label", "flip", "begin", "end", "piece_off", "grp_off", "grp_reads")


def declare(lib):
    """argument types of the demux entries (a missing symbol is an AttributeError: the library is older than this module)"""
    return capi.bind(lib, ("vc_demux_default_params", "vc_demux", "vc_demux_last_error", "vc_demux_release"))


def default_params(lib=None, **kw):
    lib = declare(lib or capi.load_hip())
    return capi.params_from_defaults(VcDemuxParams, lib.vc_demux_default_params, PARAMS, "demux", kw)


class DemuxResult(dict):
    """The arrays of one vc_demux call, named and typed like the fields of vc_demux_out (pc_bases / pc_quals as bytes or None,
    all_dist / all_end None without ALL_HITS), the call's counters under "stats" and its flags under "flags"; the keys are
    attributes too."""
    __getattr__ = dict.__getitem__

    def piece(self, r):
        """(bases, qualities or None) kept of read r"""
        a, b = int(self["piece_off"][r]), int(self["piece_off"][r + 1])
        return self["pc_bases"][a:b], (self["pc_quals"][a:b] if self["pc_quals"] is not None else None)


def demux_reads(reads, patterns, labels=None, sides=None, quals=None, require_both=False, orient=False, all_hits=False, device=0, lib=None, **params):
    """One vc_demux call.  reads / patterns: [bytes]; labels: [P] ints below 2^20 (default: every pattern its own label); sides: [P]
    of ANY / HEAD / TAIL (default ANY); quals: [bytes] per read or None; params: fields of vc_demux_params (window,
    max_err_permille, min_margin, trim, flags -- the three booleans are or-ed into flags).  Returns a DemuxResult."""
    lib = declare(lib or capi.load_hip())
    flags = int(params.pop("flags", 0)) | (REQUIRE_BOTH if require_both else 0) | (ORIENT if orient else 0) | (ALL_HITS if all_hits else 0)
    p = default_params(lib, device=device, flags=flags, **params)
    n, P = len(reads), len(patterns)
    if (labels is not None and len(labels) != P) or (sides is not None and len(sides) != P):
        raise ValueError("as many labels and sides as patterns")
    lab = np.ascontiguousarray(np.arange(P) if labels is None else np.asarray(labels, np.int64).reshape(-1))
    sd = np.ascontiguousarray(np.zeros(P, np.int64) if sides is None else np.asarray(sides, np.int64).reshape(-1))
    if P and (lab.min() < 0 or lab.max() >= 1 << 32 or sd.min() < 0 or sd.max() > 255):
        raise ValueError("a label or a side that does not fit its field")
    lab, sd = lab.astype(np.uint32), sd.astype(np.uint8)
    rd, rd_arrays = pack(reads)                              # offsets, and the bases with one pad byte behind them
    pt, pt_arrays = pack(patterns)
    a = VcDemuxIn(n, rd.off, rd.bases, None, P, pt.off, pt.bases, _ptr(lab, C.c_uint32), _ptr(sd, C.c_uint8))
    keep = [rd_arrays, pt_arrays, lab, sd]
    if quals is not None:
        if len(quals) != n or any(len(q) != len(s) for q, s in zip(quals, reads)):
            raise ValueError("a quality string per read, of the length of its read")
        q, q_arrays = pack(quals)
        a.quals = q.bases
        keep.append(q_arrays)
    o = VcDemuxOut()
    rc = lib.vc_demux(C.byref(p), C.byref(a), C.byref(o))
    if rc != 0:
        raise RuntimeError(f"vc_demux failed ({rc}): {lib.vc_demux_last_error().decode()}")
    k = int(o.n_labels)
    res = DemuxResult(v_pat=_take(o.v_pat, 2 * n, np.uint32), v_dist=_take(o.v_dist, 2 * n, np.uint8), v_start=_take(o.v_start, 2 * n, np.uint32),
                      v_end=_take(o.v_end, 2 * n, np.uint32), v_second=_take(o.v_second, 2 * n, np.uint8), klass=_take(o.klass, n, np.uint8),
                      label=_take(o.label, n, np.uint32), flip=_take(o.flip, n, np.uint8), begin=_take(o.begin, n, np.uint32), end=_take(o.end, n, np.uint32),
                      piece_off=_take(o.piece_off, n + 1, np.uint64), grp_off=_take(o.grp_off, k + 1, np.uint64))
    res["grp_reads"] = _take(o.grp_reads, int(res["grp_off"][-1]), np.uint32)
    total = int(res["piece_off"][-1])
    res["pc_bases"] = _take(o.pc_bases, total, np.uint8).tobytes() if o.pc_bases else None
    res["pc_quals"] = _take(o.pc_quals, total, np.uint8).tobytes() if o.pc_quals else None
    res["all_dist"] = _take(o.all_dist, 2 * n * P, np.uint8) if o.all_dist else None
    res["all_end"] = _take(o.all_end, 2 * n * P, np.uint32) if o.all_end else None
    res["stats"] = dict(reads=int(o.n_reads), triples=int(o.n_triples), pieces=int(o.n_budget_pieces), accepted=int(o.n_accepted))
    res["flags"] = flags
    del keep
    return res


def groups_of(result, reads):
    """The reads of every label as read groups: a list of lists of bytes, one list per label in read order, every read cut to its
    kept range and put on the forward strand -- what poa.poa_consensus and the other POA entry points take.  The bytes are the
    device's cut; a result made without orient=True has its flipped reads reverse-complemented here.  A read of which nothing is
    kept is left out; a label without a read gives an empty list."""
    if len(reads) != len(result["klass"]):
        raise ValueError("the reads of another call")
    out = []
    for g in range(len(result["grp_off"]) - 1):
        rows = []
        for r in result["grp_reads"][int(result["grp_off"][g]):int(result["grp_off"][g + 1])]:
            piece = result.piece(int(r))[0]
            if piece:
                rows.append(piece.translate(COMPLEMENT)[::-1] if result["flip"][int(r)] and not result["flags"] & ORIENT else piece)
        out.append(rows)
    return out


def read_patterns(path):
    """A FASTA of patterns -> (patterns, labels, sides, label_names, pattern_names).  A record is named `label_name` or
    `label_name:head|tail|any`; the label names are mapped to dense labels in order of first appearance."""
    patterns, labels, sides, label_names, pattern_names = [], [], [], [], []
    for name, data, _ in seqio.read_sequences(path):
        base, sep, side = name.rpartition(":")
        if not sep:
            base, side = name, "any"
        if side not in SIDES or not base:
            raise ValueError(f"{path}: the pattern name {name!r} is not label_name or label_name:head|tail|any")
        if base not in label_names:
            label_names.append(base)
        patterns.append(bytes(data)); labels.append(label_names.index(base)); sides.append(SIDES[side]); pattern_names.append(name)
    return patterns, labels, sides, label_names, pattern_names


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
            cols += ["*"] * 4 if p == UNASSIGNED else [pattern_names[p], int(res["v_dist"][v]), int(res["v_start"][v]), int(res["v_end"][v])]
        out.append("\t".join(str(c) for c in cols) + "\n")
    return "".join(out)


def format_record(name, bases, qual):
    return f"@{name}\n{bases.decode()}\n+\n{qual.decode()}\n" if qual is not None else f">{name}\n{bases.decode()}\n"


def format_reads(names, label_names, res, rows, tag):
    """the kept pieces of the reads `rows`, FASTQ with qualities and FASTA without; tag: ` label=<name>` behind the name.  A read of
    which nothing is kept has no record."""
    out = []
    for r in rows:
        bases, qual = res.piece(int(r))
        if bases:
            lab = int(res["label"][r])
            out.append(format_record(names[r] + (f" label={label_names[lab]}" if tag and lab != UNASSIGNED else ""), bases, qual))
    return "".join(out)


def format_consensus(label_names, groups, consensus):
    """>label_name size=<n>, and the consensus, for every label with a read"""
    rows = [g for g in range(len(groups)) if groups[g]]
    return "".join(f">{label_names[g]} size={len(groups[g])}\n{seq.decode()}\n" for g, seq in zip(rows, consensus))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vechat_amd.demux", description="demultiplex, orient and trim reads by adapter, primer and "
                                 "barcode on the MI355X.  The rule is this library's own, in the spirit of cutadapt and minibar, "
                                 "not a restatement of either")
    ap.add_argument("-w", dest="window", type=int, default=150, help="bases of each read end that are searched (1..4096)")
    ap.add_argument("-e", dest="max_err", type=float, default=0.2, help="errors allowed, as a fraction of the pattern's length")
    ap.add_argument("--min-margin", type=int, default=2, help="an end is ambiguous when another label's best hit is fewer errors away")
    ap.add_argument("--trim", type=int, default=1, choices=(0, 1, 2), help="0 keep everything, 1 cut the pattern and what lies outside it, 2 keep the pattern")
    ap.add_argument("--both-ends", action="store_true", help="a read with its label at one end only stays unassigned")
    ap.add_argument("--orient", action="store_true", help="reverse-complement the reads found on the minus strand")
    ap.add_argument("--report", default=None, help="TSV, one line per read: name, class, label, flip, begin, end, and per end pattern, dist, start, end")
    ap.add_argument("--out-dir", default=None, help="one FASTQ or FASTA per label, named after it")
    ap.add_argument("-o", dest="out", default=None, help="one file with label=<name> appended to the record names (- for stdout)")
    ap.add_argument("--unassigned", default=None, help="the reads without a label")
    ap.add_argument("--consensus", default=None, help="FASTA with one POA consensus per label")
    ap.add_argument("-l", dest="algorithm", type=int, default=1, choices=(0, 1, 2), help="POA alignment: 0 local, 1 global, 2 semi-global")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("patterns")
    ap.add_argument("reads")
    a = ap.parse_args(argv)
    if not 1 <= a.window <= 4096:
        ap.error("-w must lie in 1..4096")
    if not 0.0 <= a.max_err <= 1.0:
        ap.error("-e must lie in 0..1")
    if not 0 <= a.min_margin <= 64:
        ap.error("--min-margin must lie in 0..64")
    if a.out_dir and a.out:
        ap.error("--out-dir or -o, not both")
    a.params = dict(window=a.window, max_err_permille=int(round(1000 * a.max_err)), min_margin=a.min_margin, trim=a.trim,
                    require_both=a.both_ends, orient=a.orient)
    return a


def main(argv=None, out=None):
    a = parse_args(argv)
    patterns, labels, sides, label_names, pattern_names = read_patterns(a.patterns)
    recs = seqio.read_sequences(a.reads)
    names, reads = [n for n, _, _ in recs], [d for _, d, _ in recs]
    with seqio._open(a.reads) as f:
        fastq = f.read(1) == b"@"
    quals = [q if q is not None else b"!" * len(d) for _, d, q in recs] if fastq else None
    res = demux_reads(reads, patterns, labels, sides, quals=quals, device=a.device, **a.params)
    ext = "fastq" if fastq else "fasta"
    grp = lambda g: res["grp_reads"][int(res["grp_off"][g]):int(res["grp_off"][g + 1])]
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        for g, name in enumerate(label_names):
            with open(os.path.join(a.out_dir, f"{name}.{ext}"), "w") as fw:
                fw.write(format_reads(names, label_names, res, grp(g), False))
    if a.out or out is not None:
        text = format_reads(names, label_names, res, np.nonzero(res["label"] != UNASSIGNED)[0], True)
        if out is not None:
            out.write(text)
        elif a.out == "-":
            sys.stdout.write(text)
        else:
            with open(a.out, "w") as fw:
                fw.write(text)
    if a.unassigned:
        with open(a.unassigned, "w") as fw:
            fw.write(format_reads(names, label_names, res, np.nonzero(res["label"] == UNASSIGNED)[0], False))
    if a.report:
        with open(a.report, "w") as fw:
            fw.write(format_report(names, label_names, pattern_names, res))
    if a.consensus:
        from . import poa
        groups = groups_of(res, reads)
        cons = poa.poa_consensus([g for g in groups if g], algorithm=a.algorithm, device=a.device) if any(groups) else []
        with open(a.consensus, "w") as fw:
            fw.write(format_consensus(label_names, groups, cons))
    return 0


if __name__ == "__main__":
    sys.exit(main())
