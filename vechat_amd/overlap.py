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

RECORD = np.dtype([("q_id", "<u4"), ("t_id", "<u4"), ("strand", "u1"), ("q_begin", "<u4"), ("q_end", "<u4"), ("t_begin", "<u4"),
                   ("t_end", "<u4"), ("n_anchors", "<u4"), ("score", "<i4"), ("matches", "<u4"), ("block", "<u4")])
SKETCH = np.dtype([("hash", "<u8"), ("seq", "<u4"), ("pos", "<u4"), ("strand", "u1")])
PARAMS = ("k", "w", "max_occ", "max_gap", "bandwidth", "lookback", "min_chain_score", "min_anchors", "min_overlap", "drop_internal", "same_set")
PRESETS = {"ava-ont": dict(k=15, w=5), "ava-pb": dict(k=19, w=5)}


class VcOverlapSeqs(C.Structure):
    _fields_ = [("n", C.c_uint64), ("off", C.POINTER(C.c_uint64)), ("bases", C.POINTER(C.c_uint8))]


class VcOverlapParams(C.Structure):
    _fields_ = [("device", C.c_int32)] + [(f, C.c_int32) for f in PARAMS]


class VcOverlapOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("q_id", C.POINTER(C.c_uint32)), ("t_id", C.POINTER(C.c_uint32)), ("strand", C.POINTER(C.c_uint8)),
                ("q_begin", C.POINTER(C.c_uint32)), ("q_end", C.POINTER(C.c_uint32)), ("t_begin", C.POINTER(C.c_uint32)),
                ("t_end", C.POINTER(C.c_uint32)), ("n_anchors", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_int32)),
                ("matches", C.POINTER(C.c_uint32)), ("block", C.POINTER(C.c_uint32)),
                ("n_minimizers", C.c_uint64), ("n_anchors_total", C.c_uint64), ("n_keys_total", C.c_uint64)]


class VcOverlapSketchOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("hash", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
                ("strand", C.POINTER(C.c_uint8))]


def declare(lib):
    """argument types of the overlap entries (a missing symbol is an AttributeError: the library is older than this module)"""
    lib.vc_overlap.argtypes = [C.POINTER(VcOverlapParams), C.POINTER(VcOverlapSeqs), C.POINTER(VcOverlapSeqs), C.POINTER(VcOverlapOut)]
    lib.vc_overlap.restype = C.c_int
    lib.vc_overlap_sketch.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(VcOverlapSeqs), C.POINTER(VcOverlapSketchOut)]
    lib.vc_overlap_sketch.restype = C.c_int
    lib.vc_overlap_default_params.argtypes = [C.POINTER(VcOverlapParams)]
    lib.vc_overlap_default_params.restype = None
    lib.vc_overlap_last_error.restype = C.c_char_p
    lib.vc_overlap_release.restype = None
    return lib


def default_params(lib=None, **kw):
    lib = declare(lib or capi.load_hip())
    p = VcOverlapParams()
    lib.vc_overlap_default_params(C.byref(p))
    for name, v in kw.items():
        if name != "device" and name not in PARAMS:
            raise TypeError(f"unknown overlap parameter {name!r}")
        setattr(p, name, int(v))
    return p


def pack(seqs):
    """[bytes] -> (VcOverlapSeqs, the arrays that must outlive it)"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    bases = np.frombuffer(b"".join(bytes(s) for s in seqs) + b"\0", np.uint8).copy()
    return VcOverlapSeqs(len(seqs), off.ctypes.data_as(C.POINTER(C.c_uint64)), bases.ctypes.data_as(C.POINTER(C.c_uint8))), (off, bases)


def _take(ptr, n, dtype):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)


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


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
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
            qp = qp.translate(_COMP)[::-1]
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
