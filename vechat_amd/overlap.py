"""All-vs-all read overlaps on the device, over the C ABI `vc_overlap` / `vc_overlap_sketch` (include/vechat_hip.h has the rule):
the step both rounds of the driver start with, which the reference leaves to `minimap2 -x ava-* | awk | fpa`.

  python -m vechat_amd.overlap [-x ava-ont|ava-pb] [--min-overlap N] [--min-identity F] [--threads N] targets reads > out.paf

The rule is this library's own (minimizers, seeds, colinear chains, internal matches dropped), not a restatement of minimap2.
Without --min-identity columns 10 and 11 are the chain's (anchored bases, longer span); with it every record is aligned on the
device (`vc_align`) and they are exact: alignment columns minus edit distance, and alignment columns."""
import argparse
import ctypes as C
import os
import re
import sys

import numpy as np

from . import capi
from .capi import VcOverlapOut, VcOverlapParams, VcOverlapSeqs, VcOverlapSketchOut, _take, pack

RECORD = np.dtype([("q_id", "<u4"), ("t_id", "<u4"), ("strand", "u1"), ("q_begin", "<u4"), ("q_end", "<u4"), ("t_begin", "<u4"),
                   ("t_end", "<u4"), ("n_anchors", "<u4"), ("score", "<i4"), ("matches", "<u4"), ("block", "<u4")])
SKETCH = np.dtype([("hash", "<u8"), ("seq", "<u4"), ("pos", "<u4"), ("strand", "u1")])
PARAMS = tuple(f for f, _ in VcOverlapParams._fields_[1:])
PRESETS = {"ava-ont": dict(k=15, w=5), "ava-pb": dict(k=19, w=5)}
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def declare(lib):
    """argument types of the overlap entries (a missing symbol is an AttributeError: the library is older than this module)"""
    return capi.bind(lib, ("vc_overlap_default_params", "vc_overlap", "vc_overlap_sketch", "vc_overlap_last_error", "vc_overlap_release"))


def default_params(lib=None, **kw):
    lib = declare(lib or capi.load_hip())
    return capi.params_from_defaults(VcOverlapParams, lib.vc_overlap_default_params, PARAMS, "overlap", kw)


def sketch(seqs, k=15, w=5, device=0, lib=None):
    """The minimizer table of a sequence set, sorted by (seq, pos): a record array of SKETCH."""
    lib = declare(lib or capi.load_hip())
    s, keep = pack(seqs)
    o = VcOverlapSketchOut()
    rc = lib.vc_overlap_sketch(device, k, w, C.byref(s), C.byref(o))
    if rc != 0:
        raise RuntimeError(f"vc_overlap_sketch failed ({rc}): {lib.vc_overlap_last_error().decode()}")
    n = int(o.n)
    out = np.zeros(n, SKETCH)
    for f in SKETCH.names:
        out[f] = _take(getattr(o, f), n, SKETCH[f])
    del keep
    return out


def find_overlaps(targets, queries=None, device=0, lib=None, stats=None, **params):
    """Overlaps of every query against every target ([bytes] each; queries=None: the targets against themselves, same_set) as a
    record array of RECORD ordered by (q_id, t_id, strand).  params: the fields of vc_overlap_params.  stats: a dict that
    receives the call's minimizer, anchor and key counts."""
    lib = declare(lib or capi.load_hip())
    if queries is None:
        params = dict(params, same_set=1)
    p = default_params(lib, device=device, **params)
    t, keep_t = pack(targets)
    q, keep_q = pack(queries) if queries is not None else (None, None)
    o = VcOverlapOut()
    rc = lib.vc_overlap(C.byref(p), C.byref(t), C.byref(q) if q is not None else None, C.byref(o))
    if rc != 0:
        raise RuntimeError(f"vc_overlap failed ({rc}): {lib.vc_overlap_last_error().decode()}")
    n = int(o.n)
    out = np.zeros(n, RECORD)
    for f in RECORD.names:
        out[f] = _take(getattr(o, f), n, RECORD[f])
    if stats is not None:
        stats.update(minimizers=int(o.n_minimizers), anchors=int(o.n_anchors_total), keys=int(o.n_keys_total))
    del keep_t, keep_q
    return out


_RUN = re.compile(r"(\d+)[MID]")


def identity(records, targets, queries=None, device=0, lib=None):
    """`matches` and `block` exactly, through vc_align on the overlapped pieces (the query piece oriented as it aligns):
    block = the alignment's columns, matches = columns - edit distance.  Returns a copy of the records."""
    from .align import align_pairs
    queries = targets if queries is None else queries
    out = records.copy()
    pairs = []
    for r in records:
        qp = bytes(queries[int(r["q_id"])])[int(r["q_begin"]):int(r["q_end"])]
        if r["strand"]:
            qp = qp.translate(COMPLEMENT)[::-1]
        pairs.append((qp, bytes(targets[int(r["t_id"])])[int(r["t_begin"]):int(r["t_end"])]))
    cigars, dist = align_pairs(pairs, device=device, lib=lib)
    for i, (cg, d) in enumerate(zip(cigars, dist)):
        if d < 0:
            raise RuntimeError(f"record {i}: the overlap is outside vc_align's envelope")
        cols = sum(int(x) for x in _RUN.findall(cg))
        out["block"][i] = cols
        out["matches"][i] = cols - d
    return out


def write_paf(path, records, target_names, target_lens, query_names, query_lens):
    """12 PAF columns per record (mapq 255); path: a file name or an open text file."""
    fw = open(path, "w") if isinstance(path, (str, os.PathLike)) else path
    try:
        for r in records:
            q, t = int(r["q_id"]), int(r["t_id"])
            fw.write("\t".join(str(x) for x in (query_names[q], int(query_lens[q]), int(r["q_begin"]), int(r["q_end"]), "-" if r["strand"] else "+",
                                                target_names[t], int(target_lens[t]), int(r["t_begin"]), int(r["t_end"]), int(r["matches"]),
                                                int(r["block"]), 255)) + "\n")
    finally:
        if fw is not path:
            fw.close()


def records_from_paf(path, names, what):
    """The records of a PAF file from one read of it, as the dict of arrays cluster.run and scrub.intervals_from_records take: the
    nine columns of capi.CLUSTER_RECORD_FIELDS, a read as its index in names, columns 10 and 11 as they stand.  Lines and spans are
    taken as seqio.read_paf takes them; a name that is not in names is a ValueError `<path>: <name> <what>`."""
    from . import seqio
    index = {n: i for i, n in enumerate(names)}
    rows = []
    with seqio._open(path) as f:
        for ln in f:
            if not ln.strip():
                continue
            c = ln.rstrip(b"\n").split(b"\t")
            qb, qe, tb, te = int(c[2]), int(c[3]), int(c[7]), int(c[8])
            seqio._check_spans("PAF", qb, qe, int(c[1]), tb, te)
            for name in (c[0].decode(), c[5].decode()):
                if name not in index:
                    raise ValueError(f"{path}: {name!r} {what}")
            rows.append((index[c[0].decode()], index[c[5].decode()], int(c[4] == b"-"), qb, qe, tb, te, int(c[9]), int(c[10])))
    cols = np.array(rows, np.int64).reshape(-1, 9)
    return {f: cols[:, i] for i, (f, _) in enumerate(capi.CLUSTER_RECORD_FIELDS)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vechat_amd.overlap", description="all-vs-all read overlaps on the MI355X, as PAF on stdout")
    ap.add_argument("-x", dest="preset", default="ava-ont", choices=sorted(PRESETS), help="ava-ont: k 15; ava-pb: k 19")
    ap.add_argument("--min-overlap", type=int, default=500, help="shortest block (PAF column 11) kept")
    ap.add_argument("--min-identity", type=float, default=None, help="align every record on the device and keep matches / block >= F")
    ap.add_argument("--threads", "-t", type=int, default=1, help="accepted, ignored: the work is on the device")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("targets")
    ap.add_argument("reads")
    a = ap.parse_args(argv)
    if a.min_overlap <= 0:
        ap.error("--min-overlap must be positive")
    if a.min_identity is not None and not 0.0 <= a.min_identity <= 1.0:
        ap.error("--min-identity must lie in 0..1")
    return a


def main(argv=None, out=None):
    a = parse_args(argv)
    from . import seqio
    out = out or sys.stdout
    trecs = seqio.read_sequences(a.targets)
    same = os.path.abspath(a.targets) == os.path.abspath(a.reads) or os.path.samefile(a.targets, a.reads)
    qrecs = trecs if same else seqio.read_sequences(a.reads)
    targets = [d for _, d, _ in trecs]
    queries = None if same else [d for _, d, _ in qrecs]
    recs = find_overlaps(targets, queries, device=a.device, min_overlap=a.min_overlap, **PRESETS[a.preset])
    if not same:                                             # a read that is in both files does not overlap itself (fpa --same-name)
        tn, qn = [n for n, _, _ in trecs], [n for n, _, _ in qrecs]
        recs = recs[np.array([qn[int(r["q_id"])] != tn[int(r["t_id"])] for r in recs], bool)] if len(recs) else recs
    if a.min_identity is not None and len(recs):
        recs = identity(recs, targets, queries, device=a.device)
        # integers: matches / block >= F  <=>  matches >= F * block, decided in the float the awk filter of the reference uses
        recs = recs[(recs["block"] >= a.min_overlap) & (recs["matches"].astype(np.float64) >= a.min_identity * recs["block"].astype(np.float64))]
    write_paf(out, recs, [n for n, _, _ in trecs], [len(d) for d in targets], [n for n, _, _ in qrecs], [len(d) for _, d, _ in qrecs])
    return 0


if __name__ == "__main__":
    sys.exit(main())
