"""Clustering of reads into POA groups on the device, over the C ABI `vc_cluster` (include/vechat_hip.h has the rule): raw reads in,
groups out, consensus per group, without leaving the package.

  python -m vechat_amd.cluster [-x ava-ont|ava-pb] [--min-overlap N] [--min-cover F] [--either] [--min-identity F] [--min-size N]
                               [--by-size] [--longest-first] [--paf FILE] [--tsv FILE] [--consensus FILE [-l 0|1|2]] [--device D] reads

A record of the overlapper links its two reads when it is long enough, identical enough and covers enough of both reads (or, with
--either, of one); the clusters are the connected components of the links, every read with the strand that puts it into the
orientation of the cluster's first read.  The rule is this library's own -- single linkage on qualified overlaps -- and restates
no other tool.  Without --paf the overlaps are this package's own (vechat_amd.overlap on the device); nothing here computes on the
CPU what the device computes, and without a GPU the call fails."""
import argparse
import ctypes as C
import sys

import numpy as np

from . import capi
from .capi import VcClusterIn, VcClusterOut, VcClusterParams, _take
from .overlap import COMPLEMENT, PRESETS

NONE = 0xFFFFFFFF
PARAMS = tuple(f for f, _ in VcClusterParams._fields_[1:])
RECORD_FIELDS = capi.CLUSTER_RECORD_FIELDS


def declare(lib):
    """argument types of the cluster entries (a missing symbol is an AttributeError: the library is older than this module)"""
    return capi.bind(lib, ("vc_cluster_default_params", "vc_cluster", "vc_cluster_last_error", "vc_cluster_release"))


def default_params(lib=None, **kw):
    lib = declare(lib or capi.load_hip())
    return capi.params_from_defaults(VcClusterParams, lib.vc_cluster_default_params, PARAMS, "cluster", kw)


def run(lengths, records, device=0, lib=None, **params):
    """One vc_cluster call.  lengths: [n]; records: the structured array of overlap.find_overlaps, or a dict of arrays with the nine
    fields q_id, t_id, strand, q_begin, q_end, t_begin, t_end, matches, block, in any order.  Returns a dict of numpy arrays named
    and typed like the fields of vc_cluster_out plus the call's counters under "stats"."""
    lib = declare(lib or capi.load_hip())
    p = default_params(lib, device=device, **params)
    lens = np.ascontiguousarray(np.asarray(lengths, np.int64).astype(np.uint32))
    cols = []
    for f, t in RECORD_FIELDS:
        c = np.asarray(records[f], np.int64).reshape(-1)
        if c.size and (c.min() < 0 or c.max() >= 1 << (8 * C.sizeof(t))):
            raise ValueError(f"a record whose {f} does not fit its field")
        cols.append(np.ascontiguousarray(c.astype(np.uint8 if t is C.c_uint8 else np.uint32)))
    m = len(cols[0])
    if any(len(c) != m for c in cols):
        raise ValueError("record arrays of different lengths")
    a = VcClusterIn(len(lens), lens.ctypes.data_as(C.POINTER(C.c_uint32)), m, *[c.ctypes.data_as(C.POINTER(t)) for c, (_, t) in zip(cols, RECORD_FIELDS)])
    o = VcClusterOut()
    rc = lib.vc_cluster(C.byref(p), C.byref(a), C.byref(o))
    if rc != 0:
        raise RuntimeError(f"vc_cluster failed ({rc}): {lib.vc_cluster_last_error().decode()}")
    n, k = len(lens), int(o.n_clusters)
    res = dict(cl_off=_take(o.cl_off, k + 1, np.uint64))
    res.update(members=_take(o.members, int(res["cl_off"][-1]), np.uint32), cl_root=_take(o.cl_root, k, np.uint32),
               cl_twisted=_take(o.cl_twisted, k, np.uint8), cluster=_take(o.cluster, n, np.uint32), strand=_take(o.strand, n, np.uint8))
    res["stats"] = dict(records=m, links=int(o.n_links), rounds=int(o.n_rounds), components=int(o.n_components), kept=k)
    del cols, lens
    return res


def cluster_reads(reads, preset="ava-ont", min_identity=None, overlap_params=None, device=0, lib=None, **params):
    """Overlap the reads ([bytes]) against themselves on the device and cluster them: the dict of run().  The overlapper runs with its
    default drop_internal = 1, so the records' ends are moved out to the read ends, which is what a cover test wants.  With
    min_identity (a fraction) every record is aligned first (overlap.identity) so that matches and block are exact, and
    min_identity_permille is set from it.  overlap_params: further fields of vc_overlap_params; params: fields of vc_cluster_params."""
    from . import overlap
    ov = overlap.find_overlaps(reads, None, device=device, lib=lib, **dict(PRESETS[preset], **(overlap_params or {})))
    if min_identity is not None:
        if len(ov):
            ov = overlap.identity(ov, reads, None, device=device, lib=lib)
        params = dict(params, min_identity_permille=int(round(1000 * min_identity)))
    return run([len(s) for s in reads], ov, device=device, lib=lib, **params)


def groups_of(result, reads):
    """The kept clusters as read groups: a list of lists of bytes, one list per cluster in member order, every member with
    strand == 1 reverse-complemented -- what poa.poa_consensus and the other POA entry points take."""
    off, members, strand = result["cl_off"], result["members"], result["strand"]
    out = []
    for c in range(len(off) - 1):
        rows = members[int(off[c]):int(off[c + 1])]
        out.append([bytes(reads[int(r)]).translate(COMPLEMENT)[::-1] if strand[int(r)] else bytes(reads[int(r)]) for r in rows])
    return out


def format_tsv(names, result):
    """one line per read: name, cluster (`*` for none), strand (`+`, `-`, or `?` in a twisted cluster)"""
    out = []
    for r, name in enumerate(names):
        c = int(result["cluster"][r])
        twisted = c != NONE and result["cl_twisted"][c]
        out.append(f"{name}\t{'*' if c == NONE else c}\t{'?' if twisted else '-' if result['strand'][r] else '+'}\n")
    return "".join(out)


def format_consensus(names, result, consensus):
    """>cluster_<i> size=<n> root=<name of the root read>, and the consensus"""
    out = []
    for c, seq in enumerate(consensus):
        size = int(result["cl_off"][c + 1]) - int(result["cl_off"][c])
        out.append(f">cluster_{c} size={size} root={names[int(result['cl_root'][c])]}\n{seq.decode()}\n")
    return "".join(out)


def records_from_paf(path, names):
    """the records of a PAF file as the dict of arrays run() takes: columns 10 and 11 as they stand (overlap.records_from_paf)"""
    from . import overlap
    return overlap.records_from_paf(path, names, "is not a read of the input")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vechat_amd.cluster", description="cluster reads into POA groups on the MI355X: single "
                                 "linkage on qualified overlaps, every read with its strand.  The rule is this library's own and "
                                 "restates no other tool")
    ap.add_argument("-x", dest="preset", default="ava-ont", choices=sorted(PRESETS), help="the overlapper's preset (ava-ont: k 15; ava-pb: k 19)")
    ap.add_argument("--min-overlap", type=int, default=500, help="shortest block (PAF column 11) that links two reads")
    ap.add_argument("--min-cover", type=float, default=0.8, help="a linking record covers at least this fraction of both reads")
    ap.add_argument("--either", action="store_true", help="... of one of its reads is enough (a short read contained in a long one)")
    ap.add_argument("--min-identity", type=float, default=None, help="align every record on the device and link at matches / block >= F")
    ap.add_argument("--min-size", type=int, default=2, help="smallest cluster kept")
    ap.add_argument("--by-size", action="store_true", help="number the clusters by size descending, not by their first read")
    ap.add_argument("--longest-first", action="store_true", help="members by length descending: the longest read is the POA backbone")
    ap.add_argument("--paf", default=None, help="records from this PAF file instead of the device overlapper")
    ap.add_argument("--tsv", default=None, help="one line per read: name, cluster (* for none), strand (+, -, ? in a twisted cluster)")
    ap.add_argument("--consensus", default=None, help="FASTA with one POA consensus per cluster")
    ap.add_argument("-l", dest="algorithm", type=int, default=1, choices=(0, 1, 2), help="POA alignment: 0 local, 1 global, 2 semi-global")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("reads")
    a = ap.parse_args(argv)
    if a.min_overlap < 0 or a.min_size < 1:
        ap.error("--min-overlap must not be negative and --min-size must be positive")
    if not 0.0 <= a.min_cover <= 1.0 or (a.min_identity is not None and not 0.0 <= a.min_identity <= 1.0):
        ap.error("--min-cover and --min-identity must lie in 0..1")
    a.params = dict(min_overlap=a.min_overlap, min_cover_permille=int(round(1000 * a.min_cover)), cover_both=0 if a.either else 1,
                    min_size=a.min_size, by_size=int(a.by_size), longest_first=int(a.longest_first))
    return a


def main(argv=None, out=None):
    a = parse_args(argv)
    from . import seqio
    recs = seqio.read_sequences(a.reads)
    names, reads = [n for n, _, _ in recs], [d for _, d, _ in recs]
    if a.paf is None:
        res = cluster_reads(reads, preset=a.preset, min_identity=a.min_identity, device=a.device, **a.params)
    else:
        params = dict(a.params, min_identity_permille=int(round(1000 * a.min_identity))) if a.min_identity is not None else a.params
        res = run([len(s) for s in reads], records_from_paf(a.paf, names), device=a.device, **params)
    if a.consensus:
        from . import poa
        cons = poa.poa_consensus(groups_of(res, reads), algorithm=a.algorithm, device=a.device)
        with open(a.consensus, "w") as fw:
            fw.write(format_consensus(names, res, cons))
    text = format_tsv(names, res)
    if a.tsv:
        with open(a.tsv, "w") as fw:
            fw.write(text)
    elif out is not None:
        out.write(text)
    elif not a.consensus:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
