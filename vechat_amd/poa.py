"""Consensus of read groups on the device: spoa's public flow (AlignmentEngine::Create, Align + Graph::AddAlignment per
sequence in the order given, GenerateConsensus) for every group of a batch, over the C ABI `vc_poa_run` / `vc_poa_run_gaps`
(schedule 2 of vechat_amd/csrc/vc_large.hip; include/vechat_hip.h has the semantics).  Local (kSW), global (kNW) and
semi-global (kOV) alignment with linear, affine or convex gaps, the subtype chosen from the gap scores as spoa chooses it
(gap_model); no window rules.  No CPU path: without a device the calls raise.

    python -m vechat_amd.poa [-m 5] [-n -4] [-g -8] [--gap-extend E] [--gap-open2 Q] [--gap-extend2 C] [-l 0|1|2] [-r 0|1|2]
                             [--coverage] [--both-strands] [--gfa | --gfa-consensus] [--graphviz FILE]
                             [--align QUERIES --align-out FILE [--align-both-strands]]
                             [--correct FILE [--min-confidence D] [--min-support S] [--prune-rounds K]]
                             [--save-graphs FILE] [--from-graphs FILE] [--spans FILE] [--device D] FILE [FILE ...]

prints, for every FASTA / FASTQ (.gz) file in argument order, the consensus of its records in the record format of spoa's `-r 0`,
or with -r 1 / -r 2 the multiple sequence alignment of its records as FASTA (`>name` / row, with -r 2 a last row `>Consensus`;
spoa's src/main.cpp:326-335).  -r is given once (spoa's may be repeated).  --coverage adds the tag `CV:B:I,c1,c2,...` to the
`-r 0` header: per consensus base the number of records through its node and the nodes aligned to it (spoa's
GenerateConsensus(&summary, false)).  spoa's GFA output is spelt --gfa (its -r 3) and --gfa-consensus (its -r 4, with the
consensus path) here, and its -d / --dot is spelt --graphviz FILE (the spellings -r 3, -r 4, -d and --dot stay refused): the
partial order graph itself, from vc_poa_run_graph (poa_graph(), PoaGraph.to_gfa / to_dot), byte for byte what spoa's PrintGfa
(src/main.cpp:120-200) and Graph::PrintDot (src/graph.cpp:746-803) write.  --gfa / --gfa-consensus replace the -r 0 output and
exclude -r 1 / -r 2 / --coverage; --graphviz goes with every output and writes FILE for the first input file and FILE.2,
FILE.3, ... for the others.  spoa's -s /
--strand-ambiguous is spelt --both-strands here (those two spellings stay refused): every record is aligned as given and
reverse-complemented, and the better strand is added, ties going forward (spoa's src/main.cpp:287-304; vc_poa_run_strand,
poa_consensus_strands(), poa_msa(strand_ambiguous=True)).  It goes with every -r and with --coverage and changes no output
format: spoa prints nothing about strands there either, and a row shows the bytes that were kept.
poa_msa() is the same over groups in memory (vc_poa_run_msa).
--align QUERIES --align-out FILE aligns every record of QUERIES against the finished graph of every input file without adding it
(spoa's engine->Align(sequence, graph, &score); vc_poa_run_align, poa_align()) and writes FILE (align_tsv); the output on stdout
is unchanged, and with the consensus or the graph as that output the groups are built once, in the same call.  --align-both-strands tries every query on both strands and reports the better, ties as given.
--correct FILE writes every record of every input file back with its errors removed and its variants kept: VeChat's
variation-aware correction on the group's graph (prune by confidence and support, largest component, re-weight and prune again,
then the record's local alignment against what is left; vc_poa_run_correct, poa_correct()), as FASTA, one record per input
record under its own name, in input order, a record that aligns nowhere with an empty sequence line.  The output on stdout is
unchanged.  --min-confidence / --min-support / --prune-rounds default to the reference's 0.22 / 0.19 / 3.  It does not go
with -r 1 / -r 2, --gfa*, --graphviz, --both-strands or --align: those describe the unpruned graph and stay with their own calls.
--save-graphs FILE stores the finished graph of every input file, with the state a group goes on from, in one .npz file
(PoaGraph.save; vc_poa_run_from), and --from-graphs FILE starts from such a file instead of from nothing: input file k then holds
the records to ADD to stored graph k (poa_extend), and with no input file at all nothing is added and the groups carry the names
of the files they were stored from.  Both go with the consensus output, --both-strands and --align (which then runs against the
stored graphs with no build, poa_align(graphs=...)), and with each other; not with -r 1 / -r 2, --coverage, --gfa*, --graphviz or
--correct, which name records that a stored graph no longer has.
--spans FILE aligns the records it lists against a part of their file's graph only (spoa's Graph::Subgraph / UpdateAlignment;
vc_poa_run_spans, the spans= keyword of poa_consensus, poa_consensus_strands, poa_msa and poa_graph): tab-separated lines of input
file name, record name, begin, end -- inclusive positions on the file's first record --, records not listed meeting the whole
graph; a file or record that does not exist and a record listed twice are errors (parse_spans).  It goes with every -r, --coverage,
--both-strands, --gfa* and --graphviz; not with --align, --correct, --save-graphs or --from-graphs.
The files are read with the project's reader (vechat_amd.seqio), which upper-cases the bases and counts an all-'!' quality string
as none (src/sequence.cpp).  spoa's own command line keeps both verbatim (src/main.cpp:306-310 takes the quality overload for any
non-empty quality string), so for lower-case / soft-masked input, or FASTQ whose qualities are all '!', the two print different
consensus sequences.  poa_consensus() takes sequences and qualities as given.  With both strands spoa complements a kept forward
record twice, which turns u / U into T and lower-case IUPAC letters into upper case (include/vechat_hip.h); since the reader
upper-cases, on the command line only U is affected by that round trip.  spoa's -e / -q / -c are spelt --gap-extend /
--gap-open2 / --gap-extend2 here, and the gaps stay linear unless they are given (spoa's own command line defaults to convex gaps,
-g -8 -e -6 -q -10 -c -4).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import capi

ALGORITHMS = {"local": 0, "global": 1, "semi-global": 2}          # spoa::AlignmentType kSW, kNW, kOV
_STATUS = {capi.VC_WIN_INVALID: "VC_WIN_INVALID (input the reference throws on)",
           capi.VC_WIN_OVERFLOW: "VC_WIN_OVERFLOW (the device memory cannot hold it)"}


class PoaError(RuntimeError):
    """A failed vc_poa_run (rc, the library's message), or groups that were not computed (groups: {index: status})."""

    def __init__(self, msg, rc=None, groups=None):
        super().__init__(msg)
        self.rc = rc
        self.groups = groups or {}


def _entry(lib, name):
    """the entry `name` of a loaded library; a library named by VECHAT_HIP_LIB may predate it (capi.load_hip)"""
    if not hasattr(lib, name):
        raise PoaError(f"this libvechat_hip.so has no {name}: it was built before the entry point existed; rebuild it")
    return getattr(lib, name)


def algorithm_code(algorithm):
    """0 / 1 / 2 or "local" / "global" / "semi-global" -> spoa::AlignmentType"""
    if isinstance(algorithm, str):
        if algorithm not in ALGORITHMS:
            raise ValueError(f"algorithm must be one of {sorted(ALGORITHMS)} or 0 / 1 / 2, not {algorithm!r}")
        return ALGORITHMS[algorithm]
    if isinstance(algorithm, (int, np.integer)) and not isinstance(algorithm, bool) and int(algorithm) in (0, 1, 2):
        return int(algorithm)
    raise ValueError(f"algorithm must be 0, 1, 2 or one of {sorted(ALGORITHMS)}, not {algorithm!r}")


def gap_model(g, e=None, q=None, c=None):
    """spoa's subtype rule (AlignmentEngine::Create, alignment_engine.cpp:15-69) -> ("linear" | "affine" | "convex", g, e, q, c)
    with the scores the engine then uses.  Left out, e = g, q = g and c = e, as in spoa's shorter overloads."""
    e = g if e is None else e
    q = g if q is None else q
    c = e if c is None else c
    if g >= e:
        return "linear", g, g, q, c
    if g <= q or e >= c:
        return "affine", g, e, g, e
    return "convex", g, e, q, c


def _bytes(x, what):
    if isinstance(x, str):
        return x.encode("ascii")
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    raise TypeError(f"a {what} is str or bytes, not {type(x).__name__}")


def _member(m):
    """a sequence, or a (sequence, quality or None) pair -> (bytes, bytes | None)"""
    if isinstance(m, (tuple, list)):
        if len(m) != 2:
            raise ValueError("a group member is a sequence or a (sequence, quality or None) pair")
        seq, qual = m
    else:
        seq, qual = m, None
    seq = _bytes(seq, "sequence")
    if qual is None:
        return seq, None
    qual = _bytes(qual, "quality string")
    if len(qual) != len(seq):                     # spoa throws: "sequence and weights are of unequal size" (graph.cpp:191-196)
        raise ValueError(f"quality string of {len(qual)} bytes for a sequence of {len(seq)}")
    return seq, qual


def group_batch(groups):
    """groups (list of lists of sequences or (sequence, quality or None) pairs) -> capi.Batch, one window per group, sequences in
    the order given.  seq_begin / seq_end / win_fasta are zeros: vc_poa_run ignores them."""
    wso, so, hq, bases, quals = [0], [0], [], [], []
    for g in groups:
        if isinstance(g, (str, bytes)):
            raise TypeError("a group is a list of sequences, not a single sequence")
        for m in g:
            seq, qual = _member(m)
            bases.append(seq)
            quals.append(qual if qual is not None else bytes(len(seq)))
            so.append(so[-1] + len(seq))
            hq.append(0 if qual is None else 1)
        wso.append(len(hq))
    n = len(hq)
    return capi.Batch(np.array(wso, np.uint32), np.array(so, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32),
                      np.array(hq, np.uint8), np.frombuffer(b"".join(bases), np.uint8), np.frombuffer(b"".join(quals), np.uint8),
                      np.zeros(len(groups), np.uint8))


def racon_spans(backbone_len, positions):
    """The reference's rule for which layers span their window (window.cpp:207-208): offset = int(0.01 * backbone_len), and a
    member whose begin < offset and end > backbone_len - offset is aligned against the whole graph.  positions: per member a
    (begin, end) pair of inclusive positions on sequence 0, or None -> the list for spans=: None for the members that span (and
    for those given as None), (begin, end) for the others.  The library itself applies no such rule (include/vechat_hip.h)."""
    offset = int(0.01 * backbone_len)
    out = []
    for p in positions:
        if p is None:
            out.append(None)
            continue
        begin, end = p
        out.append(None if begin < offset and end > backbone_len - offset else (int(begin), int(end)))
    return out


def span_arrays(groups, spans):
    """spans (per group None or a list with one entry per member, each None or an inclusive (begin, end) on sequence 0 of the group)
    -> (begin, end) uint32 arrays with one entry per sequence of group_batch(groups), VC_POA_SPAN_NONE where there is no span; None
    when no member has a span (the call is then the plain one).  The entry of a group's first member is not read by the library and
    is stored as none.  ValueError for what vc_poa_run_spans refuses: begin > end, end beyond sequence 0, and malformed entries."""
    if spans is None:
        return None
    if len(spans) != len(groups):
        raise ValueError(f"{len(spans)} span lists for {len(groups)} groups")
    begin, end, found = [], [], False
    for w, (g, sp) in enumerate(zip(groups, spans)):
        n = len(g)
        if sp is None:
            sp = [None] * n
        if isinstance(sp, (str, bytes)) or len(sp) != n:
            raise ValueError(f"group {w}: {len(sp)} spans for {n} members (one entry per member, None or (begin, end))")
        length0 = len(_member(g[0])[0]) if n else 0
        for k, x in enumerate(sp):
            if x is None or k == 0:
                begin.append(capi.VC_POA_SPAN_NONE); end.append(capi.VC_POA_SPAN_NONE)
                continue
            if isinstance(x, (str, bytes)) or len(x) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in x):
                raise ValueError(f"group {w}, member {k}: a span is None or a pair of integers (begin, end), not {x!r}")
            b, e = int(x[0]), int(x[1])
            if b < 0 or b > e:
                raise ValueError(f"group {w}, member {k}: span ({b}, {e}) needs 0 <= begin <= end")
            if e >= length0:
                raise ValueError(f"group {w}, member {k}: span ({b}, {e}) ends beyond sequence 0 of its group ({length0} bases)")
            begin.append(b); end.append(e)
            found = True
    return (np.array(begin, np.uint32), np.array(end, np.uint32)) if found else None


def _no_spans(spans, what):
    if spans is not None:
        raise ValueError(f"{what} takes no spans: positions on sequence 0 are node ids only in a group that one call builds from "
                         "nothing (include/vechat_hip.h, vc_poa_run_spans)")


def weight_arrays(groups, weights):
    """weights (per group None or a list with one entry per member: None -- what the member's quality says, or 1 --, an int in
    0 .. 2^32 - 1 for every base of the member, or one int per base) -> (mode uint8, seq_weight uint32, base_weight uint32): mode and
    seq_weight with one entry per sequence of group_batch(groups), base_weight at the batch's base offsets; None when no member has
    a weight (the call is then the plain one).  ValueError, naming group and member, for anything else, a wrong length (spoa's
    "sequence and weights are of unequal size") or a value out of uint32."""
    if weights is None:
        return None
    if len(weights) != len(groups):
        raise ValueError(f"{len(weights)} weight lists for {len(groups)} groups")
    mode, seq_w, base_w, found = [], [], [], False
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    for w, (g, wt) in enumerate(zip(groups, weights)):
        n = len(g)
        if wt is None:
            wt = [None] * n
        if isinstance(wt, (str, bytes)) or not hasattr(wt, "__len__") or len(wt) != n:
            raise ValueError(f"group {w}: weights for {n} members need one entry per member (None, an int or one int per base)")
        for k, x in enumerate(wt):
            length = len(_member(g[k])[0])
            if x is None:
                mode.append(0); seq_w.append(0); base_w.append(np.zeros(length, np.uint32))
                continue
            found = True
            if is_int(x):
                if not 0 <= int(x) <= 0xFFFFFFFF:
                    raise ValueError(f"group {w}, member {k}: weight {int(x)} is not in 0 .. 2^32 - 1")
                mode.append(1); seq_w.append(int(x)); base_w.append(np.zeros(length, np.uint32))
                continue
            if isinstance(x, (str, bytes)) or not hasattr(x, "__len__") or not all(is_int(v) for v in x):
                raise ValueError(f"group {w}, member {k}: a weight is None, an int or a sequence of ints, not {x!r}")
            if len(x) != length:
                raise ValueError(f"group {w}, member {k}: {len(x)} weights for {length} bases (sequence and weights are of unequal size)")
            if any(not 0 <= int(v) <= 0xFFFFFFFF for v in x):
                raise ValueError(f"group {w}, member {k}: a per-base weight is not in 0 .. 2^32 - 1")
            mode.append(2); seq_w.append(0); base_w.append(np.array([int(v) for v in x], np.uint32).reshape(length))
    if not found:
        return None
    return (np.array(mode, np.uint8), np.array(seq_w, np.uint32), np.concatenate([np.zeros(0, np.uint32)] + base_w).astype(np.uint32))


def _no_weights(weights, what, profile=False):
    if weights is not None or profile:
        raise ValueError(f"{what} takes neither weights nor the profile: they belong to the call that builds a group from nothing "
                         "(include/vechat_hip.h, vc_poa_run_weighted)")


class Profile:
    """One group's per-base profile of its consensus (spoa's GenerateConsensus(&summary, true)): consensus (bytes), codes (bytes:
    the group's distinct bytes in order of first appearance), counts (numpy uint32, shape (len(codes) + 1, len(consensus)): row k
    the members that carry codes[k] in the column of each consensus base, the last row those that span it with a gap) and status."""
    __slots__ = ("consensus", "codes", "counts", "status")

    def __init__(self, consensus, codes, counts, status):
        self.consensus, self.codes, self.counts, self.status = consensus, codes, counts, status


def _profile_results(po, n, cons, status):
    res = []
    for w in range(n):
        nc, c = int(po.n_codes[w]), cons[w]
        codes = C.string_at(C.addressof(po.codes.contents) + int(po.code_off[w]), nc) if nc else b""
        k, at = (nc + 1) * len(c), int(po.prof_off[w])
        counts = _table(C.cast(C.addressof(po.counts.contents) + 4 * at, C.POINTER(C.c_uint32)), k) if k else np.zeros(0, np.uint32)
        res.append(Profile(c, codes, counts.reshape(nc + 1, len(c)), int(status[w])))
    return res


def _result_buffers(batch, stored_nodes=0):
    """-> (consensus bytes, offsets, status, VcResult over them, the batch as a struct whose seq_begin / seq_end / win_fasta are NULL)
    stored_nodes: the nodes of the graphs the groups start from (vc_poa_run_from), which the consensus may run through as well"""
    n = batch.n_windows
    cons = np.zeros(max(int(batch.bases.size) + stored_nodes, 1), np.uint8)   # a group's consensus is never longer than its sequences
    off = np.zeros(n + 1, np.uint64)
    status = np.zeros(max(n, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    return cons, off, status, r, vb


class _Outputs:
    """what _run copied out of one call; an output that was not asked for is None"""
    __slots__ = ("cons", "status", "msas", "graphs", "scores", "scores_rev", "queries", "profiles")


def _per_group(x, wso):
    return [x[wso[w]:wso[w + 1]].copy() for w in range(len(wso) - 1)]


def _graph_in(graphs):
    """stored graphs (PoaGraph made with resumable=True) -> (capi.VcPoaGraphIn, the arrays it points into: keep them alive)"""
    for g in graphs:
        if not isinstance(g, PoaGraph) or not g.resumable:
            raise ValueError("a graph to start from must come from poa_graph(..., resumable=True), poa_extend or PoaGraph.load: "
                             "without the aligned lists and the member count a group cannot go on (include/vechat_hip.h)")
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.zeros(0, dt)] + [np.asarray(x, dt) for x in xs]), dt)
    offs = lambda xs: np.concatenate([[0], np.cumsum([int(x) for x in xs])]).astype(np.uint64)

    def csr(local, counts):                 # per group nodes + 1 local offsets -> one table, every group rebased behind the one before
        base = offs(counts)
        return cat([np.asarray(o, np.uint64) + base[w] for w, o in enumerate(local)], np.uint64)

    keep = dict(
        n_members=np.array([g.n_members for g in graphs], np.uint32), n_nodes=np.array([g.n_nodes for g in graphs], np.uint32),
        node_off=offs(g.n_nodes for g in graphs), node_base=cat([g.node_base for g in graphs], np.uint8),
        rank_to_node=cat([g.rank_to_node for g in graphs], np.uint32),
        out_off=csr([g.out_off for g in graphs], [g.edge_head.size for g in graphs]),
        edge_head=cat([g.edge_head for g in graphs], np.uint32), edge_weight=cat([g.edge_weight for g in graphs], np.int64),
        al_off=csr([g.al_off for g in graphs], [g.al_node.size for g in graphs]), al_node=cat([g.al_node for g in graphs], np.uint32),
        path_first=offs(g.path_member.size for g in graphs), path_member=cat([g.path_member for g in graphs], np.uint32),
        path_reversed=cat([g.path_reversed for g in graphs], np.uint8),
        path_off=offs(n for g in graphs for n in np.diff(g.path_off)), path_node=cat([g.path_node for g in graphs], np.uint32))
    ct = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64, np.dtype(np.int64): C.c_int64}
    return capi.VcPoaGraphIn(len(graphs), **{k: v.ctypes.data_as(C.POINTER(ct[v.dtype])) for k, v in keep.items()}), keep


def _run(batch, params, *, lib=None, msa_flags=None, strands=False, strand_scores=True, graph=False, qbatch=None, align_flags=0,
         start=None, state=False, spans=None, weights=None, profile=False):
    """One library call on a capi.Batch (its seq_begin / seq_end / win_fasta are passed as NULL) with the outputs asked for:
    msa_flags (capi.VC_POA_* bits, None: no vc_poa_msa_out), strands (spoa's -s; strand_scores: with the score arrays), graph,
    qbatch + align_flags (the queries of vc_poa_run_align).  The entry is the first of vc_poa_run_align (queries), _graph, _strand,
    _msa that the request needs, else vc_poa_run_gaps (capi.VcPoaGapParams) or vc_poa_run (capi.VcPoaParams).  Everything is
    copied out of the library's buffers -> _Outputs.  Raises PoaError, naming the entry, on a library error.
    start (a list of resumable PoaGraph, one per group of the batch) and state (with graph: the graphs come back resumable) go
    through vc_poa_run_from; every other request takes the entry it always took.
    spans ((begin, end): two uint32 arrays, one entry per sequence of the batch, span_arrays) goes through vc_poa_run_spans with
    the outputs asked for (params: capi.VcPoaGapParams); not with queries, start or state.
    weights ((mode, seq_weight, base_weight), weight_arrays) and profile (-> _Outputs.profiles, a list of Profile) go through
    vc_poa_run_weighted with the outputs asked for (params: capi.VcPoaGapParams); not with queries, start, state or spans."""
    weighted = weights is not None or profile
    if weighted and (qbatch is not None or start is not None or state or spans is not None):
        raise ValueError("weights and the profile do not go with queries, stored graphs or spans (include/vechat_hip.h: out of scope "
                         "of vc_poa_run_weighted)")
    if spans is not None and (qbatch is not None or start is not None or state):
        raise ValueError("spans do not go with queries or with stored graphs (include/vechat_hip.h: out of scope of vc_poa_run_spans)")
    lib = lib or capi.load_hip()
    n = batch.n_windows
    cons, off, status, r, vb = _result_buffers(batch, sum(g.n_nodes for g in start if isinstance(g, PoaGraph)) if start is not None else 0)
    wso = [int(x) for x in batch.win_seq_off]
    o = capi.VcPoaMsaOut(flags=msa_flags) if msa_flags is not None else None
    g = capi.VcPoaGraphOut() if graph else None
    rev = sc = scr = so = None
    if strands:
        nseq = max(wso[-1], 1)
        rev = np.zeros(nseq, np.uint8)
        if strand_scores:
            sc, scr = np.zeros(nseq, np.int32), np.zeros(nseq, np.int32)
        so = C.byref(capi.VcPoaStrandOut(rev.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         *(x if x is None else x.ctypes.data_as(C.POINTER(C.c_int32)) for x in (sc, scr))))
    qv = a = st = keep = None
    first = ()                                  # what an entry takes between the parameters and the batch
    if qbatch is not None:
        qv = qbatch.as_struct()
        qv.seq_begin = qv.seq_end = qv.win_fasta = qv.seq_has_qual = qv.quals = None
        a = capi.VcPoaAlignOut(flags=align_flags)
    prof = None
    if weighted:
        name = "vc_poa_run_weighted"
        ref = lambda x: None if x is None else C.byref(x)
        win = None
        if weights is not None:
            wm, ws, wb = np.ascontiguousarray(weights[0], np.uint8), np.ascontiguousarray(weights[1], np.uint32), np.ascontiguousarray(weights[2], np.uint32)
            keep = (wm, ws, wb)                         # (the arrays the struct points into, until the call)
            win = capi.VcPoaWeightIn(wm.ctypes.data_as(C.POINTER(C.c_uint8)), ws.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     wb.ctypes.data_as(C.POINTER(C.c_uint32)))
        prof = capi.VcPoaProfileOut() if profile else None
        first = (ref(win),)
        args = (ref(o), so, ref(g), ref(prof))
    elif spans is not None:
        name = "vc_poa_run_spans"
        sb, se = (np.ascontiguousarray(x, np.uint32) for x in spans)
        keep = (sb, se)                             # (the arrays the struct points into, until the call)
        ref = lambda x: None if x is None else C.byref(x)
        first = (C.byref(capi.VcPoaSpanIn(*(x.ctypes.data_as(C.POINTER(C.c_uint32)) for x in keep))),)
        args = (ref(o), so, ref(g))
    elif start is not None or state:
        name = "vc_poa_run_from"
        if start is not None and len(start) != n:
            raise ValueError(f"{len(start)} graphs to start from for {n} groups")
        gin, keep = _graph_in(start) if start is not None else (None, None)     # (keep: the arrays gin points into, until the call)
        st = capi.VcPoaStateOut() if state else None
        ref = lambda x: None if x is None else C.byref(x)
        first, args = (ref(gin),), (ref(o), so, ref(g), ref(st), ref(qv), ref(a))
    elif qbatch is not None:
        name = "vc_poa_run_align"
        args = (so, C.byref(g) if graph else None, C.byref(qv), C.byref(a))
    elif graph:
        name, args = "vc_poa_run_graph", (C.byref(o), so, C.byref(g))
    elif strands:
        name, args = "vc_poa_run_strand", (C.byref(o), so)
    elif o is not None:
        name, args = "vc_poa_run_msa", (C.byref(o),)
    else:
        name, args = "vc_poa_run_gaps" if isinstance(params, capi.VcPoaGapParams) else "vc_poa_run", ()
    rc = _entry(lib, name)(C.byref(params), *first, C.byref(vb), C.byref(r), *args)
    if rc != 0:
        raise PoaError(f"{name} failed ({rc}): {lib.vc_poa_last_error().decode()}", rc=rc)
    x = _Outputs()
    x.cons, x.status = [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)], status[:n]
    x.msas = _msa_results(o, msa_flags, n, cons, off, wso, rev) if o is not None else None
    x.graphs = _graph_results(g, n, cons, off, x.msas if msa_flags or (strands and o is not None) else None) if graph else None
    if st is not None:
        had = [0] * n if start is None else [s.n_members for s in start]
        _state_results(st, x.graphs, [had[w] + wso[w + 1] - wso[w] for w in range(n)])
    x.scores, x.scores_rev = (_per_group(sc, wso), _per_group(scr, wso)) if sc is not None else (None, None)
    x.queries = _query_results(a, align_flags, [int(k) for k in qbatch.win_seq_off]) if qbatch is not None else None
    x.profiles = _profile_results(prof, n, x.cons, status) if prof is not None else None
    return x


def run_batch(batch, params, lib=None, spans=None, weights=None):
    """vc_poa_run (params: capi.VcPoaParams) or vc_poa_run_gaps (capi.VcPoaGapParams) on a capi.Batch (its seq_begin / seq_end /
    win_fasta are passed as NULL) -> (consensus bytes per group, status array).  Raises PoaError on a library error."""
    x = _run(batch, params, lib=lib, spans=spans, weights=weights)
    return x.cons, x.status


def _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2):
    e = gap if gap_extend is None else gap_extend
    return capi.VcPoaGapParams(device=device, algorithm=algorithm_code(algorithm), match=match, mismatch=mismatch, gap_open=gap,
                               gap_extend=e, gap_open2=gap if gap_open2 is None else gap_open2,
                               gap_extend2=e if gap_extend2 is None else gap_extend2)


def _not_computed(status, strict):
    bad = {w: int(s) for w, s in enumerate(status) if int(s) != capi.VC_WIN_OK}
    if bad and strict:
        what = ", ".join(f"{w}: {_STATUS.get(s, s)}" for w, s in list(bad.items())[:8])
        raise PoaError(f"{len(bad)} group(s) not computed: {what}{' ...' if len(bad) > 8 else ''}", groups=bad)
    return bad


def poa_consensus(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
                  gap_extend=None, gap_open2=None, gap_extend2=None, spans=None, weights=None):
    """Consensus of every group -> list of bytes.  The defaults are spoa's -m / -n / -g.  A group the device could not compute
    (VC_WIN_INVALID: the reference throws on it; VC_WIN_OVERFLOW: too large for the device memory) raises PoaError with the
    indices, or with strict=False comes back as None.
    gap_extend / gap_open2 / gap_extend2 are spoa's e / q / c: all None runs linear gaps through vc_poa_run; otherwise
    vc_poa_run_gaps with spoa's overload defaults (gap_extend = gap, gap_open2 = gap, gap_extend2 = gap_extend), whose subtype
    follows gap_model().
    spans (per group None or one entry per member, each None or an inclusive (begin, end) on sequence 0 of its group) aligns the
    members that have one against spoa's Subgraph(begin, end) only and maps the alignment back before it is added
    (vc_poa_run_spans; racon_spans applies the reference's 1 % rule to plain positions).  Without any span the call is the plain one.
    weights (per group None or one entry per member: None, an int -- spoa's AddAlignment(alignment, sequence, weight) --, or one int
    per base -- its std::vector overload --; weight_arrays) replaces a member's quality weights (vc_poa_run_weighted); not with spans.
    weights=None, or no member with a weight, is the plain call."""
    batch = group_batch(groups)
    sp = span_arrays(groups, spans)
    wt = weight_arrays(groups, weights)
    if gap_extend is None and gap_open2 is None and gap_extend2 is None and sp is None and wt is None:
        p = capi.VcPoaParams(device=device, algorithm=algorithm_code(algorithm), match=match, mismatch=mismatch, gap=gap)
    else:
        p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    cons, status = run_batch(batch, p, lib, spans=sp, weights=wt)
    bad = _not_computed(status, strict)
    return [None if w in bad else c for w, c in enumerate(cons)]


class Msa:
    """One group's result of poa_msa: rows (bytes, all of one length; '-' is a gap), members (for every row the index of the group
    member it belongs to -- an empty member has no row --, CONSENSUS_ROW for the consensus row of include_consensus), consensus
    and coverage (numpy uint32 per consensus base, or None)."""
    __slots__ = ("rows", "members", "consensus", "coverage", "reversed", "profile")

    def __init__(self, rows, members, consensus, coverage, reversed=None):
        self.rows, self.members, self.consensus, self.coverage = rows, members, consensus, coverage
        self.reversed = reversed                 # poa_msa(strand_ambiguous=True): numpy bool per group member, else None
        self.profile = None                      # poa_msa(profile=True): the group's Profile, else None

    def __iter__(self):
        return iter((self.rows, self.members, self.consensus, self.coverage))


CONSENSUS_ROW = capi.VC_POA_ROW_CONSENSUS


def _msa_results(o, flags, n, cons, off, wso, rev):
    """the Msa of every group out of a filled capi.VcPoaMsaOut (rev: the batch's strand choices, or None)"""
    res = []
    rows_base = C.addressof(o.rows.contents) if o.rows else 0
    for w in range(n):
        c0, c1 = int(off[w]), int(off[w + 1])
        rows, members, cov = [], [], None
        if o.n_rows and o.n_rows[w]:
            k, rs, at, m0 = o.n_rows[w], o.row_size[w], o.row_off[w], o.member_off[w]
            block = C.string_at(rows_base + at, k * rs)
            rows = [block[i * rs:(i + 1) * rs] for i in range(k)]
            members = [int(o.row_member[m0 + i]) for i in range(k)]
        if flags & capi.VC_POA_COVERAGE:
            cov = np.array(o.coverage[c0:c1], np.uint32) if o.coverage and c1 > c0 else np.zeros(0, np.uint32)
        res.append(Msa(rows, members, cons[c0:c1].tobytes(), cov, rev[wso[w]:wso[w + 1]].astype(bool) if rev is not None else None))
    return res


def run_batch_msa(batch, params, flags, lib=None, strands=False, spans=None, weights=None, profile=False):
    """vc_poa_run_msa (params: capi.VcPoaGapParams; flags: capi.VC_POA_* bits) on a capi.Batch -> (list of Msa, status array).
    Everything is copied out of the library's buffers before returning.  Raises PoaError on a library error.
    strands=True: vc_poa_run_strand instead -> (list of Msa with .reversed, status array, forward scores, reverse scores), the
    scores as one int32 array per group."""
    x = _run(batch, params, lib=lib, msa_flags=flags, strands=strands, spans=spans, weights=weights, profile=profile)
    for m, pr in zip(x.msas, x.profiles or ()):
        m.profile = pr
    return (x.msas, x.status, x.scores, x.scores_rev) if strands else (x.msas, x.status)


def poa_consensus_strands(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
                          gap_extend=None, gap_open2=None, gap_extend2=None, scores=False, spans=None, weights=None):
    """Consensus of every group whose members may come from either strand (spoa's -s, vc_poa_run_strand): every member is
    aligned as given and reverse-complemented and the better strand is added, ties going forward -> (list of consensus bytes,
    list of numpy bool arrays: per group, per member -- empty members included -- True where the reverse complement was kept).
    With scores=True also the forward and the reverse score of every member, two lists of int32 arrays.  The consensus is on the
    strand of the group's first non-empty member.  A kept forward member has been complemented twice: u / U count as T and
    lower-case IUPAC letters as upper case (include/vechat_hip.h).  Parameters, PoaError and strict as poa_consensus; the gap
    scores left out are spoa's overload defaults.  spans as in poa_consensus: both strands of a member meet the same subgraph, and
    the span stays in sequence 0's coordinates whichever strand is kept.  weights as in poa_consensus: a kept reverse strand is added
    with its per-base weights reversed."""
    batch = group_batch(groups)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    res, status, sc, scr = run_batch_msa(batch, p, 0, lib, strands=True, spans=span_arrays(groups, spans), weights=weight_arrays(groups, weights))
    bad = _not_computed(status, strict)
    cons = [None if w in bad else m.consensus for w, m in enumerate(res)]
    rev = [m.reversed for m in res]
    return (cons, rev, sc, scr) if scores else (cons, rev)


def poa_msa(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
            gap_extend=None, gap_open2=None, gap_extend2=None, include_consensus=False, coverage=False, strand_ambiguous=False,
            spans=None, weights=None, profile=False):
    """The multiple sequence alignment of every group (spoa's GenerateMultipleSequenceAlignment(include_consensus)) -> list of
    Msa; with coverage=True also the coverage of every consensus base (GenerateConsensus(&summary, false)).  Parameters,
    PoaError and strict as poa_consensus (a group that was not computed comes back as None with strict=False); the gap scores
    left out are spoa's overload defaults, so the default call runs linear gaps and its consensus is poa_consensus's.
    strand_ambiguous=True is spoa's -s (vc_poa_run_strand, see poa_consensus_strands): Msa.reversed then tells, per group
    member, whether the reverse complement was kept, and a row shows the kept bytes.  spans as in poa_consensus; the rows describe
    the full graph.  weights as in poa_consensus; profile=True attaches every group's Profile as Msa.profile (see poa_profile)."""
    batch = group_batch(groups)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    flags = capi.VC_POA_MSA | (capi.VC_POA_MSA_CONSENSUS if include_consensus else 0) | (capi.VC_POA_COVERAGE if coverage else 0)
    sp = span_arrays(groups, spans)
    res, status = run_batch_msa(batch, p, flags, lib, strands=strand_ambiguous, spans=sp, weights=weight_arrays(groups, weights), profile=profile)[:2]
    bad = _not_computed(status, strict)
    return [None if w in bad else m for w, m in enumerate(res)]


def poa_profile(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
                gap_extend=None, gap_open2=None, gap_extend2=None, weights=None, strand_ambiguous=False):
    """The per-base profile of every group's consensus (spoa's GenerateConsensus(&summary, true), vc_poa_run_weighted) -> list of
    Profile: for every consensus base how many members carry each code in its column and how many span it with a gap -- the table
    a consensus quality, an allele frequency or a het call is derived from --, without the alignment rows.  Weights move the
    consensus, not the counts.  Parameters, PoaError and strict as poa_consensus (a group that was not computed comes back as None
    with strict=False); weights as in poa_consensus; strand_ambiguous as in poa_msa."""
    batch = group_batch(groups)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    x = _run(batch, p, lib=lib, strands=strand_ambiguous, strand_scores=False, weights=weight_arrays(groups, weights), profile=True)
    bad = _not_computed(x.status, strict)
    return [None if w in bad else pr for w, pr in enumerate(x.profiles)]


def profile_tsv(names, profiles):
    """The bytes of --profile: per group a header line `#group, pos, base, one column per code, gaps`, then one tab-separated line per
    consensus position: group name, position, consensus base, the count of every code in codes order, the gaps."""
    out = []
    for name, pr in zip(names, profiles):
        nm = _bytes(name, "group name")
        out.append(b"#group\tpos\tbase\t" + b"".join(b"%c\t" % c for c in pr.codes) + b"gaps\n")
        cols = pr.counts.T.tolist()
        for j, col in enumerate(cols):
            out.append(b"%s\t%d\t%c\t%s\n" % (nm, j, pr.consensus[j], b"\t".join(b"%d" % v for v in col)))
    return b"".join(out)


class PoaGraph:
    """One group's partial order graph (poa_graph): numpy copies of the tables of vc_poa_graph_out (include/vechat_hip.h), with
    the offsets local to the group.  Node ids are spoa's: 0-based, in creation order.
      node_base (uint8), node_cons_pos (int32; k: the node is consensus base k, -1: not on the consensus), rank_to_node (uint32)
      out_off (int64, nodes + 1), edge_head (uint32), edge_weight (int64): node v's out-edges are out_off[v] .. out_off[v + 1]
      aligned_a, aligned_b (uint32): pairs of aligned nodes, a < b
      path_member (uint32), path_reversed (bool), path_off (int64, paths + 1), path_node (uint32): one path per member that was
        added -- an empty member has none --, in graph order; a reversed path belongs to a member whose reverse complement was kept
      cons_node (uint32), consensus (bytes); msa (an Msa, with poa_graph(msa=True), else None)
    A resumable graph (poa_graph(resumable=True), poa_extend, PoaGraph.load) also carries the state a group goes on from
    (vc_poa_state_out): al_off (int64, nodes + 1), al_node (uint32) -- node v's whole aligned list, in list order, is
    al_node[al_off[v] .. al_off[v + 1]); aligned_lists gives them as lists -- and n_members, the members the group has had so
    far, empty ones included: the next member is numbered n_members."""
    __slots__ = ("node_base", "node_cons_pos", "rank_to_node", "out_off", "edge_head", "edge_weight", "aligned_a", "aligned_b",
                 "path_member", "path_reversed", "path_off", "path_node", "cons_node", "consensus", "msa", "al_off", "al_node", "n_members")
    _ARRAYS = (("node_base", np.uint8), ("node_cons_pos", np.int32), ("rank_to_node", np.uint32), ("out_off", np.int64),
               ("edge_head", np.uint32), ("edge_weight", np.int64), ("aligned_a", np.uint32), ("aligned_b", np.uint32),
               ("path_member", np.uint32), ("path_reversed", np.bool_), ("path_off", np.int64), ("path_node", np.uint32),
               ("cons_node", np.uint32), ("al_off", np.int64), ("al_node", np.uint32))

    def __init__(self, **kw):
        self.msa = self.al_off = self.al_node = self.n_members = None
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def resumable(self):
        return self.al_off is not None and self.n_members is not None

    @property
    def aligned_lists(self):
        """-> per node the list of the nodes aligned to it, in list order (None unless resumable)"""
        if self.al_off is None:
            return None
        ao, an = self.al_off.tolist(), self.al_node.tolist()
        return [an[ao[v]:ao[v + 1]] for v in range(self.n_nodes)]

    @staticmethod
    def save(path, graphs, names=None):
        """Stores a list of resumable graphs as one .npz file at exactly `path`, numpy arrays only: every table of every graph
        back to back with a table of lengths, the consensus, n_members, and with names= one name (bytes) per graph."""
        for g in graphs:
            if not isinstance(g, PoaGraph) or not g.resumable:
                raise ValueError("only resumable graphs can be stored: poa_graph(..., resumable=True), poa_extend")
        data = {"n_members": np.array([g.n_members for g in graphs], np.uint32)}
        for k, dt in PoaGraph._ARRAYS:
            xs = [np.asarray(getattr(g, k), dt) for g in graphs]
            data[k] = np.concatenate([np.zeros(0, dt)] + xs)
            data[k + "_len"] = np.array([x.size for x in xs], np.int64)
        cons = [bytes(g.consensus) for g in graphs]
        data["consensus"] = np.frombuffer(b"".join(cons), np.uint8)
        data["consensus_len"] = np.array([len(c) for c in cons], np.int64)
        if names is not None:
            data["names"] = np.array([_bytes(x, "graph name") for x in names], dtype=np.bytes_).reshape(len(graphs))
        with open(path, "wb") as f:
            np.savez(f, **data)

    @staticmethod
    def load(path, names=False):
        """-> the list of graphs PoaGraph.save stored at `path`; with names=True (that list, their names as bytes or None)"""
        with np.load(path, allow_pickle=False) as z:
            data = {k: z[k] for k in z.files}
        graphs = [PoaGraph(n_members=int(m)) for m in data["n_members"]]
        for k, dt in PoaGraph._ARRAYS + (("consensus", np.uint8),):
            at = np.concatenate([[0], np.cumsum(data[k + "_len"])]).astype(np.int64)
            for w, g in enumerate(graphs):
                x = data[k][at[w]:at[w + 1]].astype(dt, copy=True)
                setattr(g, k, x.tobytes() if k == "consensus" else x)
        stored = [bytes(x) for x in data["names"]] if "names" in data else None
        return (graphs, stored) if names else graphs

    @property
    def n_nodes(self):
        return int(self.node_base.size)

    def edges(self):
        """-> [(tail, head, weight)] by tail id, then by position in the tail's out-list (spoa's printing order)"""
        tails = np.repeat(np.arange(self.n_nodes), np.diff(self.out_off))
        return list(zip(tails.tolist(), self.edge_head.tolist(), self.edge_weight.tolist()))

    def aligned_pairs(self):
        """-> [(a, b)], a < b"""
        return list(zip(self.aligned_a.tolist(), self.aligned_b.tolist()))

    def paths(self):
        """-> [(member, reversed, [node ids in graph order])]"""
        po, pn = self.path_off.tolist(), self.path_node.tolist()
        return [(int(m), bool(r), pn[po[k]:po[k + 1]]) for k, (m, r) in enumerate(zip(self.path_member, self.path_reversed))]

    def to_gfa(self, names, include_consensus=False):
        """The bytes of spoa's PrintGfa (src/main.cpp:120-200; its -r 3, or with include_consensus its -r 4).  names: the name of
        every group member (str or bytes), empty members included.  Tab-separated; node ids are printed + 1; a weight is printed
        as the integer it is (`ew:f:<int64>`); `ic:Z:true` marks consensus nodes and the links between two of them; a reversed
        path is printed backwards with `-` on every node.
        One deliberate difference: spoa indexes its headers and reversal flags by the i-th ADDED sequence, so after an empty
        record it prints the name of the wrong record; here a path is named by its own member."""
        on = (self.node_cons_pos >= 0).tolist()
        base, off, head, weight = self.node_base.tolist(), self.out_off.tolist(), self.edge_head.tolist(), self.edge_weight.tolist()
        out = [b"H\tVN:Z:1.0\n"]
        for v in range(self.n_nodes):
            out.append(b"S\t%d\t%c%s\n" % (v + 1, base[v], b"\tic:Z:true" if on[v] else b""))
            for k in range(off[v], off[v + 1]):
                out.append(b"L\t%d\t+\t%d\t+\tOM\tew:f:%d%s\n" % (v + 1, head[k] + 1, weight[k], b"\tic:Z:true" if on[v] and on[head[k]] else b""))
        for member, rev, path in self.paths():
            name = names[member]
            sign = b"-" if rev else b"+"
            out.append(b"P\t%s\t%s\t*\n" % (name.encode() if isinstance(name, str) else bytes(name),
                                             b",".join(b"%d%s" % (v + 1, sign) for v in (path[::-1] if rev else path))))
        if include_consensus:
            out.append(b"P\tConsensus\t%s\t*\n" % b",".join(b"%d+" % (v + 1) for v in self.cons_node.tolist()))
        return b"".join(out)

    def to_dot(self):
        """The bytes of spoa's Graph::PrintDot (src/graph.cpp:746-803; its -d FILE beside -r 0, i.e. after GenerateConsensus):
        consensus nodes filled, an edge coloured where its head follows its tail on the consensus (spoa's test is
        rank[tail] + 1 == rank[head] with -1 for a node off the consensus, kept as it is), aligned pairs dotted."""
        pos, base = self.node_cons_pos.tolist(), self.node_base.tolist()
        off, head, weight = self.out_off.tolist(), self.edge_head.tolist(), self.edge_weight.tolist()
        al = {}
        for a, b in self.aligned_pairs():
            al.setdefault(a, []).append(b)
        out = [b"digraph %d {\n  graph [rankdir = LR]\n" % self.path_member.size]
        for v in range(self.n_nodes):
            out.append(b'  %d[label = "%d - %c"%s]\n' % (v, v, base[v], b", style = filled, fillcolor = goldenrod1" if pos[v] != -1 else b""))
            for k in range(off[v], off[v + 1]):
                out.append(b'  %d -> %d [label = "%d"%s]\n' % (v, head[k], weight[k],
                                                               b", color = goldenrod1" if pos[v] + 1 == pos[head[k]] else b""))
            for b in al.get(v, ()):
                out.append(b"  %d -> %d [style = dotted, arrowhead = none]\n" % (v, b))
        out.append(b"}\n")
        return b"".join(out)


def run_batch_graph(batch, params, flags=0, lib=None, strands=False, spans=None, weights=None, profile=False):
    """vc_poa_run_graph (params: capi.VcPoaGapParams; flags: capi.VC_POA_* bits for the alignment beside it, 0: none) on a
    capi.Batch -> (list of PoaGraph, status array); strands=True builds the groups with spoa's -s and also returns the forward and
    reverse scores per group, as run_batch_msa.  PoaGraph.msa is the group's Msa (its .reversed set with strands).  Everything is
    copied out of the library's buffers before returning.  Raises PoaError on a library error."""
    x = _run(batch, params, lib=lib, msa_flags=flags, strands=strands, graph=True, spans=spans, weights=weights, profile=profile)
    return (x.graphs, x.status, x.scores, x.scores_rev) if strands else (x.graphs, x.status)


def _table(ptr, count):
    """a copy of a whole library-owned table (one view over it, no Python list between)"""
    return np.ctypeslib.as_array(ptr, shape=(count,)).copy() if count else np.zeros(0, ptr._type_)


def _graph_results(g, n, cons, off, msas=None):
    """the PoaGraph of every group out of a filled capi.VcPoaGraphOut (msas: the Msa of every group, or None)"""
    table = _table
    node_off = table(g.node_off, n + 1).astype(np.int64)
    nn = int(node_off[-1])
    out_off = table(g.out_off, nn + n).astype(np.int64)
    aligned_off, path_first = table(g.aligned_off, n + 1).astype(np.int64), table(g.path_first, n + 1).astype(np.int64)
    ne, na, npath = int(out_off[-1]) if n else 0, int(aligned_off[-1]), int(path_first[-1])
    path_off = table(g.path_off, npath + 1).astype(np.int64)
    node_base, node_cons_pos, rank_to_node = table(g.node_base, nn), table(g.node_cons_pos, nn), table(g.rank_to_node, nn)
    edge_head, edge_weight = table(g.edge_head, ne), table(g.edge_weight, ne)
    aligned_a, aligned_b = table(g.aligned_a, na), table(g.aligned_b, na)
    path_member, path_reversed = table(g.path_member, npath), table(g.path_reversed, npath).astype(bool)
    path_node, cons_node = table(g.path_node, int(path_off[-1])), table(g.cons_node, int(off[n]))
    res = []
    for w in range(n):
        n0, n1 = int(node_off[w]), int(node_off[w + 1])
        oo = out_off[n0 + w:n1 + w + 1]
        e0, e1 = int(oo[0]), int(oo[-1])
        a0, a1, p0, p1 = int(aligned_off[w]), int(aligned_off[w + 1]), int(path_first[w]), int(path_first[w + 1])
        po = path_off[p0:p1 + 1]
        c0, c1 = int(off[w]), int(off[w + 1])
        res.append(PoaGraph(node_base=node_base[n0:n1].copy(), node_cons_pos=node_cons_pos[n0:n1].copy(),
                            rank_to_node=rank_to_node[n0:n1].copy(), out_off=oo - e0,
                            edge_head=edge_head[e0:e1].copy(), edge_weight=edge_weight[e0:e1].copy(),
                            aligned_a=aligned_a[a0:a1].copy(), aligned_b=aligned_b[a0:a1].copy(),
                            path_member=path_member[p0:p1].copy(), path_reversed=path_reversed[p0:p1].copy(),
                            path_off=po - po[0], path_node=path_node[int(po[0]):int(po[-1])].copy(),
                            cons_node=cons_node[c0:c1].copy(), consensus=cons[c0:c1].tobytes(),
                            msa=msas[w] if msas is not None else None))
    return res


def _state_results(st, graphs, n_members):
    """adds the state of a filled capi.VcPoaStateOut to the PoaGraph of every group: al_off, al_node, n_members"""
    n = len(graphs)
    nn = sum(g.n_nodes for g in graphs)
    al_off = _table(st.al_off, nn + n).astype(np.int64) if n else np.zeros(0, np.int64)
    al_node = _table(st.al_node, int(al_off[-1]) if n else 0)
    at = 0
    for w, g in enumerate(graphs):
        ao = al_off[at:at + g.n_nodes + 1]
        at += g.n_nodes + 1
        g.al_off, g.al_node, g.n_members = ao - ao[0], al_node[int(ao[0]):int(ao[-1])].copy(), int(n_members[w])


def poa_graph(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
              gap_extend=None, gap_open2=None, gap_extend2=None, strand_ambiguous=False, msa=False, resumable=False, spans=None,
              weights=None):
    """The partial order graph of every group (vc_poa_run_graph) -> list of PoaGraph: nodes, weighted edges, aligned nodes, the
    path of every member and the consensus path, as spoa's GFA (-r 3 / -r 4) and dot (-d) output hold them; PoaGraph.to_gfa and
    to_dot give those bytes.  Parameters, PoaError and strict as poa_consensus (a group that was not computed comes back as None
    with strict=False); the gap scores left out are spoa's overload defaults.  strand_ambiguous=True builds the graph with spoa's
    -s (poa_consensus_strands): a member whose reverse complement was kept has a path with reversed=True.  msa=True also asks
    for the multiple sequence alignment of the same graph in the same call: PoaGraph.msa, as poa_msa() returns it.
    resumable=True (vc_poa_run_from) also returns the state a group goes on from -- aligned_lists and n_members --, so that the
    graphs can be stored (PoaGraph.save), extended (poa_extend) and queried (poa_align(graphs=...)) without building them again.
    spans as in poa_consensus; the tables describe the full graph.  Not with resumable=True (ValueError).
    weights as in poa_consensus: edge_weight holds the sums.  Not with resumable=True (ValueError)."""
    if resumable:
        _no_spans(spans, "poa_graph(resumable=True)")
        _no_weights(weights, "poa_graph(resumable=True)")
    batch = group_batch(groups)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    sp = span_arrays(groups, spans)
    if resumable:
        x = _run(batch, p, lib=lib, msa_flags=capi.VC_POA_MSA if msa else 0, strands=strand_ambiguous, graph=True, state=True)
        res, status = x.graphs, x.status
    else:
        res, status = run_batch_graph(batch, p, capi.VC_POA_MSA if msa else 0, lib, strands=strand_ambiguous, spans=sp,
                                      weights=weight_arrays(groups, weights))[:2]
    bad = _not_computed(status, strict)
    return [None if w in bad else m for w, m in enumerate(res)]


def poa_extend(graphs, groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
               gap_extend=None, gap_open2=None, gap_extend2=None, strand_ambiguous=False, msa=False, include_consensus=False,
               coverage=False, spans=None, weights=None):
    """Adds the members of groups[w] to the stored graph graphs[w] (vc_poa_run_from; spoa's AddAlignment on a live graph) -> (the
    new graphs, resumable again, the list of consensus bytes); with msa=True or coverage=True -> (graphs, consensus, list of
    Msa), the alignment of all members so far as poa_msa returns it (include_consensus as there), also at PoaGraph.msa.
    The new members are numbered from graphs[w].n_members in Msa.members and path_member; with strand_ambiguous=True they are
    added with spoa's -s and Msa.reversed tells about them alone.  With the parameters of the call that made the graphs, the
    result is byte for byte the one call on all members.  A graph made without resumable=True raises ValueError; parameters,
    PoaError and strict as poa_consensus.  spans= is refused (ValueError): in a stored graph a position on sequence 0 is no node id."""
    _no_spans(spans, "poa_extend")
    _no_weights(weights, "poa_extend")
    if len(graphs) != len(groups):
        raise ValueError(f"{len(graphs)} graphs for {len(groups)} groups")
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    want_msa = msa or coverage
    flags = (capi.VC_POA_MSA if msa else 0) | (capi.VC_POA_MSA_CONSENSUS if msa and include_consensus else 0) | (capi.VC_POA_COVERAGE if coverage else 0)
    x = _run(group_batch(groups), p, lib=lib, msa_flags=flags if want_msa or strand_ambiguous else None, strands=strand_ambiguous,
             graph=True, start=list(graphs), state=True)
    bad = _not_computed(x.status, strict)
    out = [None if w in bad else g for w, g in enumerate(x.graphs)]
    cons = [None if w in bad else c for w, c in enumerate(x.cons)]
    return (out, cons, [None if w in bad else m for w, m in enumerate(x.msas)]) if want_msa else (out, cons)


class QueryAlignment:
    """One query's result of poa_align: score and score_rev (spoa's *score as given and reverse-complemented; score_rev is None
    without both_strands), reversed (True: the reverse complement was kept, and positions count in its bytes), status
    (capi.VC_WIN_*) and pairs: an (n, 2) int32 array of (node id or -1, position or -1), spoa's Alignment, or None without pairs=."""
    __slots__ = ("score", "score_rev", "reversed", "status", "pairs")

    def __init__(self, score, score_rev, reversed, status, pairs):
        self.score, self.score_rev, self.reversed, self.status, self.pairs = score, score_rev, reversed, status, pairs

    def __iter__(self):
        return iter((self.score, self.score_rev, self.reversed, self.status, self.pairs))


def query_batch(queries):
    """queries (one list of sequences per group) -> capi.Batch of which vc_poa_run_align reads win_seq_off, seq_off and bases"""
    return group_batch([[_bytes(s, "query") for s in qs] for qs in queries])


def run_batch_align(batch, qbatch, params, flags=capi.VC_POA_ALIGN_PAIRS, lib=None, strands=False, graph=False):
    """vc_poa_run_align (params: capi.VcPoaGapParams; flags: capi.VC_POA_ALIGN_* bits) on a capi.Batch of groups and one of
    queries, window w of qbatch being the queries of group w -> (consensus bytes per group, status array, per group the list of
    QueryAlignment, list of PoaGraph or None).  strands=True builds the groups with spoa's -s; graph=True also asks for the
    graph tables of the same call.  Everything is copied out of the library's buffers before returning.  Raises PoaError on a
    library error."""
    x = _run(batch, params, lib=lib, strands=strands, strand_scores=False, graph=graph, qbatch=qbatch, align_flags=flags)
    return x.cons, x.status, x.queries, x.graphs


def _query_results(a, flags, wq):
    """per group the list of QueryAlignment out of a filled capi.VcPoaAlignOut (wq: the query batch's win_seq_off)"""
    nq = int(a.n_queries)
    st, sc = _table(a.status, nq), _table(a.score, nq)
    both = bool(flags & capi.VC_POA_ALIGN_STRANDS)
    scr, rv = (_table(a.score_rev, nq), _table(a.reversed, nq)) if both else (None, None)
    pairs = None
    if flags & capi.VC_POA_ALIGN_PAIRS:
        po = _table(a.pair_off, nq + 1).astype(np.int64)
        pairs = np.stack([_table(a.pair_node, int(po[-1])), _table(a.pair_pos, int(po[-1]))], axis=1) if nq else np.zeros((0, 2), np.int32)
    return [[QueryAlignment(int(sc[k]), int(scr[k]) if both else None, bool(rv[k]) if both else False, int(st[k]),
                            pairs[int(po[k]):int(po[k + 1])].copy() if pairs is not None else None) for k in range(wq[w], wq[w + 1])]
            for w in range(len(wq) - 1)]


def poa_align(groups=None, queries=None, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
              gap_extend=None, gap_open2=None, gap_extend2=None, pairs=True, both_strands=False, strand_ambiguous=False, graph=False,
              graphs=None, spans=None, weights=None):
    """Aligns queries against the finished graphs of their groups without adding them (spoa's engine->Align(query, graph,
    &score); vc_poa_run_align): queries[w] is the list of queries of groups[w] -> per group a list of QueryAlignment; with
    graph=True -> (that, list of PoaGraph of the same call), whose node ids the pairs refer to.  pairs=False returns the scores
    only (no backtrack runs).  both_strands aligns every query as given and reverse-complemented and keeps the better, ties as
    given (VC_POA_ALIGN_STRANDS); strand_ambiguous is the build's -s, as in poa_graph.  Parameters, PoaError and strict as
    poa_consensus: a group that was not computed raises, or with strict=False its queries carry its status.  ValueError when
    the number of query lists differs from the number of groups.
    graphs= (resumable PoaGraph, one per query list) aligns against stored graphs with no build in the call (vc_poa_run_from):
    give either groups or graphs; both together first add groups[w] to graphs[w] and then align, and graph=True then returns the
    extended graphs, resumable again.  spans= is refused (ValueError): neither the build of this call nor its queries take them."""
    _no_spans(spans, "poa_align")
    _no_weights(weights, "poa_align")
    if queries is None:
        raise ValueError("poa_align needs queries")
    if groups is None and graphs is None:
        raise ValueError("poa_align needs groups to build, or graphs to align against (or both, to extend the graphs first)")
    if groups is None:
        groups = [[] for _ in graphs]
    if len(queries) != len(groups):
        raise ValueError(f"{len(queries)} query lists for {len(groups)} groups")
    if graphs is not None and len(graphs) != len(groups):
        raise ValueError(f"{len(graphs)} graphs for {len(groups)} groups")
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    flags = (capi.VC_POA_ALIGN_PAIRS if pairs else 0) | (capi.VC_POA_ALIGN_STRANDS if both_strands else 0)
    if graphs is not None:
        x = _run(group_batch(groups), p, lib=lib, strands=strand_ambiguous, strand_scores=False, graph=graph, qbatch=query_batch(queries),
                 align_flags=flags, start=list(graphs), state=graph)
        status, res, out = x.status, x.queries, x.graphs
    else:
        _, status, res, out = run_batch_align(group_batch(groups), query_batch(queries), p, flags, lib, strands=strand_ambiguous, graph=graph)
    bad = _not_computed(status, strict)
    if graph:
        return res, [None if w in bad else g for w, g in enumerate(out)]
    return res


class Assignment:
    """One query's result of poa_assign: best_group and second_group (indices into the groups, -1 where no pair was ranked),
    their scores (0 where none), reversed (True: the reverse complement scored higher against best_group; always False without
    both_strands) and status (capi.VC_WIN_*: OVERFLOW if any pair of the query overflowed, else INVALID if any was invalid)."""
    __slots__ = ("best_group", "best_score", "second_group", "second_score", "reversed", "status")

    def __init__(self, best_group, best_score, second_group, second_score, reversed, status):
        self.best_group, self.best_score, self.second_group, self.second_score = best_group, best_score, second_group, second_score
        self.reversed, self.status = reversed, status

    def __iter__(self):
        return iter((self.best_group, self.best_score, self.second_group, self.second_score, self.reversed, self.status))

    def __repr__(self):
        return "Assignment(best_group=%d, best_score=%d, second_group=%d, second_score=%d, reversed=%r, status=%d)" % tuple(self)


def run_batch_assign(batch, qbatch, params, flags=0, lib=None, start=None):
    """vc_poa_run_assign (params: capi.VcPoaGapParams; flags: capi.VC_POA_ASSIGN_* bits) on a capi.Batch of groups and one of
    queries, every sequence of qbatch being a query against every group; start: resumable PoaGraph, one per group, or None ->
    (consensus bytes per group, status array of the groups, list of Assignment, the (queries, groups) int32 score table or None,
    the uint8 pair status table or None).  Everything is copied out of the library's buffers.  Raises PoaError on a library error."""
    lib = lib or capi.load_hip()
    run = _entry(lib, "vc_poa_run_assign")
    n = batch.n_windows
    if start is not None and len(start) != n:
        raise ValueError(f"{len(start)} graphs to start from for {n} groups")
    cons, off, status, r, vb = _result_buffers(batch, sum(g.n_nodes for g in start if isinstance(g, PoaGraph)) if start is not None else 0)
    gin, keep = _graph_in(start) if start is not None else (None, None)     # (keep: the arrays gin points into, until the call)
    qv = qbatch.as_struct()
    qv.seq_begin = qv.seq_end = qv.win_fasta = qv.seq_has_qual = qv.quals = None
    a = capi.VcPoaAssignOut(flags=flags)
    rc = run(C.byref(params), None if gin is None else C.byref(gin), C.byref(vb), C.byref(r), C.byref(qv), C.byref(a))
    del keep
    if rc != 0:
        raise PoaError(f"vc_poa_run_assign failed ({rc}): {lib.vc_poa_last_error().decode()}", rc=rc)
    nq, ng = int(a.n_queries), int(a.n_groups)
    st, bg, bs = _table(a.status, nq), _table(a.best_group, nq), _table(a.best_score, nq)
    sg, ss = _table(a.second_group, nq), _table(a.second_score, nq)
    rv = _table(a.reversed, nq) if flags & capi.VC_POA_ASSIGN_STRANDS else np.zeros(nq, np.uint8)
    res = [Assignment(int(bg[k]), int(bs[k]), int(sg[k]), int(ss[k]), bool(rv[k]), int(st[k])) for k in range(nq)]
    table = pst = None
    if flags & capi.VC_POA_ASSIGN_SCORES:
        table, pst = _table(a.scores, nq * ng).reshape(nq, ng), _table(a.pair_status, nq * ng).reshape(nq, ng)
    return [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)], status[:n], res, table, pst


def poa_assign(groups=None, queries=None, *, graphs=None, both_strands=False, scores=False, algorithm="global", match=5, mismatch=-4,
               gap=-8, device=0, strict=True, lib=None, gap_extend=None, gap_open2=None, gap_extend2=None, spans=None, weights=None):
    """Scores every query against EVERY group without adding it (spoa's engine->Align(query, graph, &score); vc_poa_run_assign)
    and assigns it: queries is one flat list of sequences -> one Assignment per query, the best and the second group by score
    (ties to the lower index; a group with an empty graph is scored but never ranked).  With scores=True -> (that, the
    (queries, groups) int32 numpy array of every pair's score, the kept strand's with both_strands).  both_strands scores every
    query as given and reverse-complemented and keeps the better, ties as given.  Only scores are computed -- no alignment is
    kept -- so a pair stores the graph's live rows alone; follow up with poa_align on the winners for the pairs.
    graphs= (resumable PoaGraph) scores against stored graphs; with groups too, groups[w] is first added to graphs[w].
    Parameters, PoaError and strict as poa_consensus: a group that was not computed raises, or with strict=False its pairs carry
    its status.  spans= and weights= are refused (ValueError), as by poa_align."""
    _no_spans(spans, "poa_assign")
    _no_weights(weights, "poa_assign")
    if queries is None:
        raise ValueError("poa_assign needs queries")
    if groups is None and graphs is None:
        raise ValueError("poa_assign needs groups to build, or graphs to score against (or both, to extend the graphs first)")
    if groups is None:
        groups = [[] for _ in graphs]
    if graphs is not None and len(graphs) != len(groups):
        raise ValueError(f"{len(graphs)} graphs for {len(groups)} groups")
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    flags = (capi.VC_POA_ASSIGN_STRANDS if both_strands else 0) | (capi.VC_POA_ASSIGN_SCORES if scores else 0)
    _, status, res, table, _ = run_batch_assign(group_batch(groups), query_batch([list(queries)]), p, flags, lib,
                                                start=list(graphs) if graphs is not None else None)
    _not_computed(status, strict)
    return (res, table) if scores else res


class Corrected:
    """One group's result of poa_correct: consensus (bytes; of the unpruned graph, poa_consensus's), reads (the corrected bytes of
    every member, in member order; empty where the member aligns nowhere or is empty), scores (numpy int32: the local score of
    every member against the final graph) and status (numpy uint8, capi.VC_WIN_* per member)."""
    __slots__ = ("consensus", "reads", "scores", "status")

    def __init__(self, consensus, reads, scores, status):
        self.consensus, self.reads, self.scores, self.status = consensus, reads, scores, status

    def __iter__(self):
        return iter((self.consensus, self.reads, self.scores, self.status))


def _prune_params(min_confidence, min_support, prune_rounds):
    """the checks of vc_poa_run_correct, before any batch is made"""
    if isinstance(prune_rounds, bool) or not isinstance(prune_rounds, (int, np.integer)) or not 1 <= int(prune_rounds) < 2 ** 32:
        raise ValueError(f"prune_rounds must be an integer >= 1, not {prune_rounds!r}")
    for name, v in (("min_confidence", min_confidence), ("min_support", min_support)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not float(v) >= 0:
            raise ValueError(f"{name} must be a number >= 0, not {v!r}")
    return capi.VcPoaPruneParams(float(min_confidence), float(min_support), int(prune_rounds))


def run_batch_correct(batch, params, prune, lib=None):
    """vc_poa_run_correct (params: capi.VcPoaGapParams; prune: capi.VcPoaPruneParams) on a capi.Batch -> (list of Corrected, status
    array per group).  Everything is copied out of the library's buffers before returning.  Raises PoaError on a library error."""
    lib = lib or capi.load_hip()
    run = _entry(lib, "vc_poa_run_correct")
    n = batch.n_windows
    cons, off, status, r, vb = _result_buffers(batch)
    co = capi.VcPoaCorrectOut()
    rc = run(C.byref(vb), C.byref(params), C.byref(prune), C.byref(r), C.byref(co))
    if rc != 0:
        raise PoaError(f"vc_poa_run_correct failed ({rc}): {lib.vc_poa_last_error().decode()}", rc=rc)
    ns = int(co.n_seqs)
    st, sc, po = _table(co.status, ns), _table(co.score, ns), _table(co.corr_off, ns + 1).astype(np.int64)
    corr = _table(co.corr, int(po[-1])).tobytes()
    wso = [int(x) for x in batch.win_seq_off]
    res = [Corrected(cons[int(off[w]):int(off[w + 1])].tobytes(), [corr[int(po[s]):int(po[s + 1])] for s in range(wso[w], wso[w + 1])],
                     sc[wso[w]:wso[w + 1]].copy(), st[wso[w]:wso[w + 1]].copy()) for w in range(n)]
    return res, status[:n]


def poa_correct(groups, algorithm="global", match=5, mismatch=-4, gap=-8, device=0, strict=True, lib=None, *,
                gap_extend=None, gap_open2=None, gap_extend2=None, min_confidence=0.22, min_support=0.19, prune_rounds=3, spans=None,
                weights=None):
    """Haplotype-aware correction of every member of every group (vc_poa_run_correct; the flow is in include/vechat_hip.h): the
    group's graph is built as poa_consensus builds it, pruned by confidence and support down to its largest component,
    re-weighted by the members and pruned again (prune_rounds - 1 times, with the call's engine), and every member is read off its
    local alignment against what is left -- its errors removed, its variants kept -> list of Corrected (consensus, reads, scores,
    status).  The defaults are the reference's.  Parameters, PoaError and strict as poa_consensus: a group that was not computed
    raises, or with strict=False comes back as None; a member the device could not align carries its own status in
    Corrected.status and has an empty read.  ValueError for prune_rounds < 1 or a threshold that is negative or NaN, and for spans=
    (the rounds rebuild and renumber the graph)."""
    _no_spans(spans, "poa_correct")
    _no_weights(weights, "poa_correct")
    prune = _prune_params(min_confidence, min_support, prune_rounds)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    res, status = run_batch_correct(group_batch(groups), p, prune, lib)
    bad = _not_computed(status, strict)
    return [None if w in bad else c for w, c in enumerate(res)]


class Haplotypes:
    """One group's result of poa_haplotypes: consensus (one bytes per haplotype, largest first), sizes (members per haplotype),
    members (per group member its haplotype, None for an empty member), sites ((column, major, minor, n_major, n_minor) with the
    alleles as bytes, b"-" a gap), status."""
    __slots__ = ("consensus", "sizes", "members", "sites", "status")

    def __init__(self, consensus, sizes, members, sites, status):
        self.consensus, self.sizes, self.members, self.sites, self.status = consensus, sizes, members, sites, status


def hap_params(max_haplotypes=2, min_reads=2, min_fraction=0.25, indels=False, rounds=4):
    """the checks of vc_poa_run_haplotypes' own parameters, before any batch is made; min_fraction becomes permille here, once"""
    for name, v, lo, hi in (("max_haplotypes", max_haplotypes, 1, capi.VC_POA_HAP_MAX), ("min_reads", min_reads, 1, 2 ** 32 - 1),
                            ("rounds", rounds, 1, 2 ** 32 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {v!r}")
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating)) or not 0 <= float(min_fraction) <= 1:
        raise ValueError(f"min_fraction must be a number in 0..1, not {min_fraction!r}")
    return capi.VcPoaHapParams(int(max_haplotypes), int(min_reads), int(round(1000 * float(min_fraction))), int(rounds),
                               capi.VC_POA_HAP_INDELS if indels else 0)


def run_batch_haplotypes(batch, params, hap, lib=None):
    """vc_poa_run_haplotypes (params: capi.VcPoaGapParams; hap: capi.VcPoaHapParams) on a capi.Batch -> (consensus bytes per group,
    status array, list of Haplotypes, the raw tables as a dict of numpy arrays).  Everything is copied out of the library's buffers
    before returning.  Raises PoaError on a library error."""
    lib = lib or capi.load_hip()
    run = _entry(lib, "vc_poa_run_haplotypes")
    n = batch.n_windows
    cons, off, status, r, vb = _result_buffers(batch)
    o = capi.VcPoaHapOut()
    rc = run(C.byref(params), C.byref(hap), C.byref(vb), C.byref(r), C.byref(o))
    if rc != 0:
        raise PoaError(f"vc_poa_run_haplotypes failed ({rc}): {lib.vc_poa_last_error().decode()}", rc=rc)
    wso = [int(x) for x in batch.win_seq_off]
    group_cons = [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)]
    if n == 0:
        return group_cons, status[:0], [], {}
    hf, so = _table(o.hap_first, n + 1).astype(np.int64), _table(o.site_off, n + 1).astype(np.int64)
    nh, ns = int(hf[-1]), int(so[-1])
    co = _table(o.cons_off, nh + 1).astype(np.int64)
    raw = dict(n_haps=_table(o.n_haps, n), hap_first=hf, hap_size=_table(o.hap_size, nh), cons_off=co, cons=_table(o.cons, int(co[-1])),
               hap_of=_table(o.hap_of, wso[-1]), site_off=so, site_col=_table(o.site_col, ns), site_major=_table(o.site_major, ns),
               site_minor=_table(o.site_minor, ns), site_n_major=_table(o.site_n_major, ns), site_n_minor=_table(o.site_n_minor, ns),
               bytes=int(o.bytes))
    hb = raw["cons"].tobytes()
    res = []
    for w in range(n):
        hs = range(int(hf[w]), int(hf[w + 1]))
        res.append(Haplotypes(
            [hb[int(co[h]):int(co[h + 1])] for h in hs], [int(raw["hap_size"][h]) for h in hs],
            [None if int(x) == capi.VC_POA_HAP_NONE else int(x) for x in raw["hap_of"][wso[w]:wso[w + 1]]],
            [(int(raw["site_col"][k]), bytes([int(raw["site_major"][k])]), bytes([int(raw["site_minor"][k])]), int(raw["site_n_major"][k]),
              int(raw["site_n_minor"][k])) for k in range(int(so[w]), int(so[w + 1]))],
            int(status[w])))
    return group_cons, status[:n], res, raw


def poa_haplotypes(groups, max_haplotypes=2, min_reads=2, min_fraction=0.25, indels=False, rounds=4, algorithm="global", match=5,
                   mismatch=-4, gap=-8, device=0, strict=True, lib=None, *, gap_extend=None, gap_open2=None, gap_extend2=None):
    """The haplotypes of every group (vc_poa_run_haplotypes; the rule is in include/vechat_hip.h): the group's graph is built as
    poa_consensus builds it, the columns in which at least two alleles reach min_reads members and min_fraction of the members
    that span them become sites, the members are clustered by their alleles at the sites into at most max_haplotypes clusters,
    and every cluster gets the consensus of the graph restricted to its members -> list of Haplotypes.  indels=True lets a gap be
    an allele.  Parameters, PoaError and strict as poa_consensus: a group that was not computed raises, or with strict=False
    comes back as None.  ValueError for a parameter outside its range."""
    hap = hap_params(max_haplotypes, min_reads, min_fraction, indels, rounds)
    p = _gap_params(algorithm, match, mismatch, gap, device, gap_extend, gap_open2, gap_extend2)
    _, status, res, _ = run_batch_haplotypes(group_batch(groups), p, hap, lib)
    bad = _not_computed(status, strict)
    return [None if w in bad else h for w, h in enumerate(res)]


def haplotype_fasta(group_names, results):
    """The text of --haplotypes: >GROUP_hapK members=N and the haplotype's consensus, groups in input order"""
    return b"".join(b">%s_hap%d members=%d\n%s\n" % (_bytes(g, "group name"), k, n, c)
                    for g, h in zip(group_names, results) if h is not None for k, (c, n) in enumerate(zip(h.consensus, h.sizes)))


def haplotype_members_tsv(group_names, records, results):
    """The text of --hap-members: file, read name, haplotype (or - for a member that was not added)"""
    return b"".join(b"%s\t%s\t%s\n" % (_bytes(g, "group name"), _bytes(name, "record name"), b"-" if m is None else b"%d" % m)
                    for g, recs, h in zip(group_names, records, results) if h is not None for (name, _, _), m in zip(recs, h.members))


def haplotype_sites_tsv(group_names, results):
    """The text of --hap-sites: file, column, major, minor, n_major, n_minor"""
    return b"".join(b"%s\t%d\t%s\t%s\t%d\t%d\n" % (_bytes(g, "group name"), c, a, b, na, nb)
                    for g, h in zip(group_names, results) if h is not None for c, a, b, na, nb in h.sites)


def corrected_fasta(records, results):
    """The text of --correct: records[w] the (name, data, quality) records of group w, results[w] its Corrected -> FASTA, one
    record per member under its own name, groups in input order; an empty correction has an empty sequence line."""
    return b"".join(b">%s\n%s\n" % (_bytes(name, "record name"), read)
                    for recs, c in zip(records, results) for (name, _, _), read in zip(recs, c.reads))


_STATUS_NAME = {capi.VC_WIN_OK: b"OK", capi.VC_WIN_OVERFLOW: b"OVERFLOW", capi.VC_WIN_INVALID: b"INVALID"}


def align_tsv(names, files, results):
    """The text of --align-out: one tab-separated line per (query, group), queries outermost -- query name, group file, status,
    score (the kept strand's), strand (+ / -), pairs as node:pos,... with * for -1, or * for an empty alignment.
    results[w][k]: the QueryAlignment of query k against group w."""
    out = []
    for k, name in enumerate(names):
        for w, f in enumerate(files):
            r = results[w][k]
            prs = b"*" if r.pairs is None or len(r.pairs) == 0 else \
                b",".join(b"%s:%s" % (b"*" if v < 0 else b"%d" % v, b"*" if p < 0 else b"%d" % p) for v, p in r.pairs.tolist())
            out.append(b"%s\t%s\t%s\t%d\t%s\t%s\n" % (_bytes(name, "query name"), _bytes(f, "file name"),
                                                      _STATUS_NAME.get(r.status, b"%d" % r.status),
                                                      r.score_rev if r.reversed else r.score, b"-" if r.reversed else b"+", prs))
    return b"".join(out)


def assign_tsv(names, files, results):
    """The text of --assign-out, beside align_tsv: one tab-separated line per query -- query name, the best group's file, its
    score, the second group's file, its score, strand (+ / -, against the best group), status; * and 0 where no group was ranked.
    results[k]: the Assignment of query k."""
    f = [_bytes(x, "file name") for x in files]
    return b"".join(b"%s\t%s\t%d\t%s\t%d\t%s\t%s\n" % (_bytes(name, "query name"), f[r.best_group] if r.best_group >= 0 else b"*", r.best_score,
                                                      f[r.second_group] if r.second_group >= 0 else b"*", r.second_score,
                                                      b"-" if r.reversed else b"+", _STATUS_NAME.get(r.status, b"%d" % r.status))
                    for name, r in zip(names, results))


def assign_scores_tsv(names, files, table):
    """The text of --assign-scores: a header line `query` and the group files, then per query its name and its score against every group"""
    head = b"query" + b"".join(b"\t" + _bytes(x, "file name") for x in files) + b"\n"
    return head + b"".join(_bytes(name, "query name") + b"".join(b"\t%d" % v for v in row) + b"\n" for name, row in zip(names, table.tolist()))


def parse_spans(text, files, records):
    """The file of --spans: tab-separated lines `group-file-name, member-name, begin, end` (inclusive positions on the first record
    of that file; empty lines and lines starting with # are skipped) -> the list for spans=, one list per input file with None
    for every member that is not listed.  files: the input file names as given on the command line, records[w] the (name, data,
    quality) records of file w.  ValueError for a malformed line, a file or member that does not exist (or a member name that
    two records of the file share), and a (file, member) listed twice."""
    index = {}
    for w, f in enumerate(files):
        if _bytes(f, "file name") in index:
            raise ValueError(f"--spans: the input file {f} is given twice, so its name does not tell the groups apart")
        index[_bytes(f, "file name")] = w
    members = []
    for recs in records:
        names = {}
        for k, (name, _, _) in enumerate(recs):
            names.setdefault(_bytes(name, "record name"), []).append(k)
        members.append(names)
    spans = [[None] * len(recs) for recs in records]
    seen = set()
    for no, line in enumerate(_bytes(text, "span file").split(b"\n"), 1):
        line = line.rstrip(b"\r")
        if not line.strip() or line.startswith(b"#"):
            continue
        cols = line.split(b"\t")
        if len(cols) != 4 or not cols[2].isdigit() or not cols[3].isdigit():
            raise ValueError(f"--spans line {no}: expected group-file-name, member-name, begin, end separated by tabs")
        f, name = cols[0], cols[1]
        if f not in index:
            raise ValueError(f"--spans line {no}: no input file named {f.decode(errors='replace')}")
        w = index[f]
        ks = members[w].get(name, [])
        if len(ks) != 1:
            raise ValueError(f"--spans line {no}: {f.decode(errors='replace')} has {'no' if not ks else 'more than one'} record named "
                             f"{name.decode(errors='replace')}")
        if (w, ks[0]) in seen:
            raise ValueError(f"--spans line {no}: {name.decode(errors='replace')} of {f.decode(errors='replace')} is listed twice")
        seen.add((w, ks[0]))
        spans[w][ks[0]] = (int(cols[2]), int(cols[3]))
    return spans


def parse_weights(text, files, records):
    """The file of --weights: tab-separated lines `group-file-name, member-name, weight`, weight one integer (for every base of the
    record) or a comma list with one integer per base (empty lines and lines starting with # are skipped) -> the list for weights=,
    one list per input file with None for every member that is not listed.  files, records and the ValueErrors as parse_spans; a
    comma list of the wrong length or a value beyond 2^32 - 1 is a ValueError too."""
    index = {}
    for w, f in enumerate(files):
        if _bytes(f, "file name") in index:
            raise ValueError(f"--weights: the input file {f} is given twice, so its name does not tell the groups apart")
        index[_bytes(f, "file name")] = w
    members = []
    for recs in records:
        names = {}
        for k, (name, _, _) in enumerate(recs):
            names.setdefault(_bytes(name, "record name"), []).append(k)
        members.append(names)
    weights = [[None] * len(recs) for recs in records]
    seen = set()
    for no, line in enumerate(_bytes(text, "weight file").split(b"\n"), 1):
        line = line.rstrip(b"\r")
        if not line.strip() or line.startswith(b"#"):
            continue
        cols = line.split(b"\t")
        if len(cols) != 3 or not all(v.isdigit() for v in cols[2].split(b",")):
            raise ValueError(f"--weights line {no}: expected group-file-name, member-name, weight (an integer or a comma list) separated by tabs")
        f, name = cols[0], cols[1]
        if f not in index:
            raise ValueError(f"--weights line {no}: no input file named {f.decode(errors='replace')}")
        w = index[f]
        ks = members[w].get(name, [])
        if len(ks) != 1:
            raise ValueError(f"--weights line {no}: {f.decode(errors='replace')} has {'no' if not ks else 'more than one'} record named "
                             f"{name.decode(errors='replace')}")
        if (w, ks[0]) in seen:
            raise ValueError(f"--weights line {no}: {name.decode(errors='replace')} of {f.decode(errors='replace')} is listed twice")
        seen.add((w, ks[0]))
        vals = [int(v) for v in cols[2].split(b",")]
        if any(v > 0xFFFFFFFF for v in vals):
            raise ValueError(f"--weights line {no}: a weight is not in 0 .. 2^32 - 1")
        if b"," in cols[2] and len(vals) != len(records[w][ks[0]][1]):
            raise ValueError(f"--weights line {no}: {len(vals)} weights for the {len(records[w][ks[0]][1])} bases of {name.decode(errors='replace')}")
        weights[w][ks[0]] = vals if b"," in cols[2] else vals[0]
    return weights


def parse_args(argv=None):
    ap = argparse.ArgumentParser(
        prog="python -m vechat_amd.poa",
        description="Partial-order consensus of each FASTA/FASTQ(.gz) file on the device, as spoa computes it (one file = one group; "
                    "records in file order, quality strings as weights; read as the polisher reads them: upper-cased, an all-'!' quality "
                    "string counts as none). Gaps are linear unless --gap-extend / --gap-open2 / --gap-extend2 are given (spoa's -e / -q / "
                    "-c, which this command does not take as such); spoa's own defaults are -g -8 --gap-extend -6 --gap-open2 -10 "
                    "--gap-extend2 -4 (convex gaps).")
    ap.add_argument("-m", type=int, default=5, help="score for matching bases (default 5)")
    ap.add_argument("-n", type=int, default=-4, help="score for mismatching bases (default -4)")
    ap.add_argument("-g", type=int, default=-8, help="gap opening penalty, <= 0 (default -8)")
    ap.add_argument("--gap-extend", type=int, default=None, metavar="E",
                    help="gap extension penalty, <= 0 (spoa's -e; default: -g, linear gaps)")
    ap.add_argument("--gap-open2", type=int, default=None, metavar="Q",
                    help="gap opening penalty of the second affine model, <= 0 (spoa's -q; default: -g)")
    ap.add_argument("--gap-extend2", type=int, default=None, metavar="C",
                    help="gap extension penalty of the second affine model, <= 0 (spoa's -c; default: --gap-extend)")
    ap.add_argument("-l", type=int, default=0, choices=(0, 1, 2), help="alignment mode: 0 local (SW), 1 global (NW), 2 semi-global (OV); default 0")
    ap.add_argument("-r", type=int, default=0, choices=(0, 1, 2),
                    help="result: 0 consensus (FASTA), 1 multiple sequence alignment (FASTA), 2 both, the consensus as the last row "
                         "'Consensus' (spoa's -r; given once here, and without spoa's GFA modes 3 and 4); default 0")
    ap.add_argument("--coverage", action="store_true",
                    help="with -r 0: add the tag CV:B:I,c1,c2,... to the header, the coverage of every consensus base")
    ap.add_argument("--both-strands", action="store_true",
                    help="align every record as given and reverse-complemented and add the better strand (spoa's -s / "
                         "--strand-ambiguous); the output formats are unchanged")
    ap.add_argument("--gfa", action="store_true",
                    help="print the partial order graph as GFA instead of the consensus (spoa's -r 3); not with -r 1 / -r 2 / --coverage")
    ap.add_argument("--gfa-consensus", action="store_true", help="--gfa with the consensus as a last path (spoa's -r 4)")
    ap.add_argument("--graphviz", metavar="FILE", default=None,
                    help="also write the graph in Graphviz dot format to FILE (spoa's -d); with several input files FILE is the "
                         "first one's and FILE.2, FILE.3, ... the others'")
    ap.add_argument("--align", metavar="QUERIES", default=None,
                    help="also align every record of QUERIES (FASTA / FASTQ) against the graph of every input file, without adding it")
    ap.add_argument("--align-out", metavar="FILE", default=None,
                    help="where --align writes: one tab-separated line per (query, group): query name, group file, status, score, "
                         "strand, pairs (node:pos,... with * for none)")
    ap.add_argument("--align-both-strands", action="store_true",
                    help="with --align: align every query as given and reverse-complemented and report the better strand")
    ap.add_argument("--assign", metavar="QUERIES", default=None,
                    help="also score every record of QUERIES (FASTA / FASTQ) against the graph of every input file, without adding it, "
                         "and report the best and the second file per record (scores only: far cheaper than --align)")
    ap.add_argument("--assign-out", metavar="FILE", default=None,
                    help="where --assign writes: one tab-separated line per query: query name, best group's file, score, second "
                         "group's file, second score, strand, status")
    ap.add_argument("--assign-both-strands", action="store_true",
                    help="with --assign: score every query as given and reverse-complemented and keep the better strand")
    ap.add_argument("--assign-scores", metavar="FILE", default=None,
                    help="with --assign: also write the score of every (query, file) pair to FILE, one tab-separated line per query")
    ap.add_argument("--correct", metavar="FILE", default=None,
                    help="also write every record, haplotype-aware corrected on its file's graph, to FILE as FASTA (the consensus on "
                         "stdout is unchanged); not with -r 1 / -r 2, --gfa*, --graphviz, --both-strands or --align")
    ap.add_argument("--min-confidence", type=float, default=0.22, metavar="D", help="with --correct: minimum confidence of an edge (default 0.22)")
    ap.add_argument("--min-support", type=float, default=0.19, metavar="S", help="with --correct: minimum support of an edge (default 0.19)")
    ap.add_argument("--prune-rounds", type=int, default=3, metavar="K", help="with --correct: number of prune rounds, >= 1 (default 3)")
    ap.add_argument("--save-graphs", metavar="FILE", default=None,
                    help="also store the finished graph of every input file in FILE (.npz), to go on from later")
    ap.add_argument("--from-graphs", metavar="FILE", default=None,
                    help="start from the graphs stored in FILE: input file k is added to graph k; without input files nothing is added")
    ap.add_argument("--spans", metavar="FILE", default=None,
                    help="align the listed records against a part of their file's graph only: tab-separated lines of input file name, "
                         "record name, begin, end (inclusive positions on the file's first record); records not listed meet the whole "
                         "graph. Not with --align, --correct, --save-graphs or --from-graphs")
    ap.add_argument("--weights", metavar="FILE", default=None,
                    help="weigh the listed records explicitly instead of by their quality: tab-separated lines of input file name, "
                         "record name, weight -- one integer for every base, or a comma list with one integer per base; records not "
                         "listed keep their quality weights. Not with --align, --correct, --spans, --save-graphs or --from-graphs")
    ap.add_argument("--profile", metavar="FILE", default=None,
                    help="also write the per-base profile of every consensus to FILE: a header line per group naming its codes, then one "
                         "tab-separated line per consensus position: group, position, base, one count per code, gaps. Not with --align, "
                         "--correct, --spans, --save-graphs or --from-graphs")
    ap.add_argument("--haplotypes", metavar="FILE", default=None,
                    help="also split every input file's records into haplotypes and write their consensus sequences to FILE as FASTA, "
                         "'>INPUT_hapK members=N' (the consensus on stdout is unchanged); only with the plain consensus output")
    ap.add_argument("--hap-members", metavar="FILE", default=None,
                    help="also write the haplotype of every record to FILE: tab-separated input file, record name, haplotype (- for an empty record)")
    ap.add_argument("--hap-sites", metavar="FILE", default=None,
                    help="also write the sites that separate the haplotypes to FILE: tab-separated input file, column, major, minor, n_major, n_minor")
    ap.add_argument("--max-haplotypes", type=int, default=2, metavar="K", help="with --haplotypes / --hap-*: at most K haplotypes per file, 1..8 (default 2)")
    ap.add_argument("--hap-min-reads", type=int, default=2, metavar="N",
                    help="with --haplotypes / --hap-*: an allele and a haplotype need N records (default 2)")
    ap.add_argument("--hap-min-fraction", type=float, default=0.25, metavar="F",
                    help="with --haplotypes / --hap-*: an allele needs the fraction F of the records that span its column (default 0.25)")
    ap.add_argument("--hap-indels", action="store_true", help="with --haplotypes / --hap-*: a gap is an allele too")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal (default 0)")
    ap.add_argument("files", nargs="*", metavar="FILE")
    a = ap.parse_args(argv)
    if not a.files and a.from_graphs is None:
        ap.error("the following arguments are required: FILE")
    return a


def main(argv=None):
    a = parse_args(argv)
    from . import seqio
    if a.coverage and a.r != 0:
        print("vechat_amd.poa: --coverage goes with -r 0", file=sys.stderr)
        return 1
    gfa = a.gfa or a.gfa_consensus
    if gfa and (a.r != 0 or a.coverage):
        print("vechat_amd.poa: --gfa / --gfa-consensus do not go with -r 1 / -r 2 / --coverage", file=sys.stderr)
        return 1
    if (a.align is None) != (a.align_out is None) or (a.align_both_strands and a.align is None):
        print("vechat_amd.poa: --align QUERIES and --align-out FILE go together (--align-both-strands with them)", file=sys.stderr)
        return 1
    if (a.assign is None) != (a.assign_out is None) or ((a.assign_both_strands or a.assign_scores is not None) and a.assign is None):
        print("vechat_amd.poa: --assign QUERIES and --assign-out FILE go together (--assign-both-strands and --assign-scores with them)",
              file=sys.stderr)
        return 1
    if a.assign is not None and (a.correct is not None or a.spans is not None or a.weights is not None or a.profile is not None):
        print("vechat_amd.poa: --assign does not go with --correct, --spans, --weights or --profile", file=sys.stderr)
        return 1
    if a.correct is not None and (a.r != 0 or gfa or a.graphviz is not None or a.both_strands or a.align is not None):
        print("vechat_amd.poa: --correct does not go with -r 1 / -r 2, --gfa / --gfa-consensus, --graphviz, --both-strands or --align "
              "(they describe the unpruned graph: run them on their own)", file=sys.stderr)
        return 1
    resume = a.save_graphs is not None or a.from_graphs is not None
    if resume and (a.r != 0 or a.coverage or gfa or a.graphviz is not None or a.correct is not None):
        print("vechat_amd.poa: --save-graphs / --from-graphs do not go with -r 1 / -r 2, --coverage, --gfa / --gfa-consensus, --graphviz "
              "or --correct", file=sys.stderr)
        return 1
    if a.spans is not None and (resume or a.correct is not None or a.align is not None):
        print("vechat_amd.poa: --spans does not go with --align, --correct, --save-graphs or --from-graphs", file=sys.stderr)
        return 1
    if (a.weights is not None or a.profile is not None) and (resume or a.correct is not None or a.align is not None or a.spans is not None):
        print("vechat_amd.poa: --weights / --profile do not go with --align, --correct, --spans, --save-graphs or --from-graphs", file=sys.stderr)
        return 1
    hap_out = a.haplotypes is not None or a.hap_members is not None or a.hap_sites is not None
    if hap_out and (a.r != 0 or a.coverage or gfa or a.graphviz is not None or a.both_strands or a.align is not None or a.assign is not None or
                    a.correct is not None or resume or a.spans is not None or a.weights is not None or a.profile is not None):
        print("vechat_amd.poa: --haplotypes / --hap-members / --hap-sites go with the consensus only (vc_poa_run_haplotypes takes no "
              "spans, weights, strands, queries or stored graphs): run the other outputs on their own", file=sys.stderr)
        return 1
    # what the command line asks for: the alignment rows or the coverage (a vc_poa_msa_out, which vc_poa_run_align does not carry),
    # the graph tables, the queries
    want_msa = a.r != 0 or a.coverage
    want_graph = gfa or a.graphviz is not None
    msa_flags = capi.VC_POA_MSA | (capi.VC_POA_MSA_CONSENSUS if a.r == 2 else 0) | (capi.VC_POA_COVERAGE if a.coverage else 0) if want_msa else 0
    msa = cons = graphs = None
    try:
        records = [list(seqio.read_sequences(f)) for f in a.files]
        groups = [[(data, qual) for _, data, qual in recs] for recs in records]
        gaps = dict(gap_extend=a.gap_extend, gap_open2=a.gap_open2, gap_extend2=a.gap_extend2)
        p = _gap_params(a.l, a.m, a.n, a.g, a.device, **gaps)
        spans = None
        if a.spans is not None:
            with open(a.spans, "rb") as f:
                spans = parse_spans(f.read(), a.files, records)
        with_spans = dict(spans=spans) if spans is not None else {}     # (a call without --spans is the call it always was)
        weights = None
        if a.weights is not None:
            with open(a.weights, "rb") as f:
                weights = parse_weights(f.read(), a.files, records)
        if weights is not None or a.profile is not None:
            # one call of vc_poa_run_weighted for everything the command line asks for, and the profile beside it
            wt = weight_arrays(groups, weights)
            x = _run(group_batch(groups), p, msa_flags=msa_flags if want_msa or want_graph or a.both_strands else None, strands=a.both_strands,
                     strand_scores=False, graph=want_graph, weights=wt, profile=a.profile is not None)
            _not_computed(x.status, True)
            if a.profile is not None:
                with open(a.profile, "wb") as f:
                    f.write(profile_tsv(a.files, x.profiles))
            if want_graph:
                graphs = x.graphs
            if want_msa:
                msa = x.msas
            elif not gfa:
                cons = x.cons
        start, names = None, a.files
        if resume:
            # one call of vc_poa_run_from: the stored graphs (or none), the records to add (or none), the queries (or none)
            start, names = PoaGraph.load(a.from_graphs, names=True) if a.from_graphs is not None else (None, None)
            if start is not None and not a.files:
                groups, names = [[] for _ in start], names or [b"graph%d" % (k + 1) for k in range(len(start))]
            else:
                names = a.files
            if start is not None and len(start) != len(groups):
                raise ValueError(f"{a.from_graphs} holds {len(start)} graphs for {len(groups)} input files")
            qrecs = list(seqio.read_sequences(a.align)) if a.align is not None else None
            flags = capi.VC_POA_ALIGN_PAIRS | (capi.VC_POA_ALIGN_STRANDS if a.align_both_strands else 0)
            x = _run(group_batch(groups), p, strands=a.both_strands, strand_scores=False, graph=a.save_graphs is not None,
                     qbatch=query_batch([[data for _, data, _ in qrecs]] * len(groups)) if qrecs is not None else None,
                     align_flags=flags, start=start, state=a.save_graphs is not None)
            _not_computed(x.status, True)
            if a.save_graphs is not None:
                PoaGraph.save(a.save_graphs, x.graphs, names)
            if qrecs is not None:
                with open(a.align_out, "wb") as f:
                    f.write(align_tsv([name for name, _, _ in qrecs], names, x.queries))
            cons = x.cons
        elif a.correct is not None:
            # one call: the consensus of the unpruned graph (with --coverage a second, plain one below) and every record corrected
            res, status = run_batch_correct(group_batch(groups), p, _prune_params(a.min_confidence, a.min_support, a.prune_rounds))
            _not_computed(status, True)
            with open(a.correct, "wb") as f:
                f.write(corrected_fasta(records, res))
            if not want_msa:
                cons = [c.consensus for c in res]
        elif hap_out:
            # one call: the consensus of every file on stdout as always, and its haplotypes into the files asked for
            hp = hap_params(a.max_haplotypes, a.hap_min_reads, a.hap_min_fraction, a.hap_indels)
            cons, status, res, _ = run_batch_haplotypes(group_batch(groups), p, hp)
            _not_computed(status, True)
            for path, text in ((a.haplotypes, lambda: haplotype_fasta(a.files, res)),
                               (a.hap_members, lambda: haplotype_members_tsv(a.files, records, res)),
                               (a.hap_sites, lambda: haplotype_sites_tsv(a.files, res))):
                if path is not None:
                    with open(path, "wb") as f:
                        f.write(text())
        if a.align is not None and not resume:
            # every query against every group.  Without rows or coverage this one call builds the groups once and gives the
            # consensus or the graph too; beside them it is a call of its own
            qrecs = list(seqio.read_sequences(a.align))
            flags = capi.VC_POA_ALIGN_PAIRS | (capi.VC_POA_ALIGN_STRANDS if a.align_both_strands else 0)
            c, status, res, gr = run_batch_align(group_batch(groups), query_batch([[data for _, data, _ in qrecs]] * len(groups)), p, flags,
                                                 strands=a.both_strands, graph=want_graph and not want_msa)
            _not_computed(status, True)
            with open(a.align_out, "wb") as f:
                f.write(align_tsv([name for name, _, _ in qrecs], a.files, res))
        if resume or weights is not None or a.profile is not None:
            pass
        elif a.align is not None and not want_msa:
            cons, graphs = (None if gfa else c), gr
        elif cons is not None:
            pass
        elif want_graph:
            # one call for everything: the graph carries the consensus, and with -r 1 / -r 2 / --coverage the alignment beside it
            arrays = dict(spans=span_arrays(groups, spans)) if spans is not None else {}
            graphs, status = run_batch_graph(group_batch(groups), p, msa_flags, strands=a.both_strands, **arrays)[:2]
            _not_computed(status, True)
            if want_msa:
                msa = [g.msa for g in graphs]
            elif not gfa:
                cons = [g.consensus for g in graphs]
        elif not want_msa:
            if a.both_strands:
                cons = poa_consensus_strands(groups, a.l, a.m, a.n, a.g, device=a.device, **gaps, **with_spans)[0]
            else:
                cons = poa_consensus(groups, a.l, a.m, a.n, a.g, device=a.device, **gaps, **with_spans)
        else:
            strands = dict(strand_ambiguous=True) if a.both_strands else {}
            msa = poa_msa(groups, a.l, a.m, a.n, a.g, device=a.device, include_consensus=a.r == 2, coverage=a.coverage, **gaps, **strands,
                          **with_spans)
        if a.assign is not None:
            # a call of its own: every query against every group (the stored graphs with the input files added, with --from-graphs)
            qrecs = list(seqio.read_sequences(a.assign))
            flags = capi.VC_POA_ASSIGN_STRANDS if a.assign_both_strands else 0
            flags |= capi.VC_POA_ASSIGN_SCORES if a.assign_scores is not None else 0
            _, status, res, table, _ = run_batch_assign(group_batch(groups), query_batch([[data for _, data, _ in qrecs]]), p, flags, start=start)
            _not_computed(status, True)
            with open(a.assign_out, "wb") as f:
                f.write(assign_tsv([name for name, _, _ in qrecs], names, res))
            if a.assign_scores is not None:
                with open(a.assign_scores, "wb") as f:
                    f.write(assign_scores_tsv([name for name, _, _ in qrecs], names, table))
        for k, g in enumerate(graphs if a.graphviz is not None else ()):
            with open(a.graphviz if k == 0 else f"{a.graphviz}.{k + 1}", "wb") as f:
                f.write(g.to_dot())
    except (PoaError, ValueError, OSError) as e:
        print(f"vechat_amd.poa: {e}", file=sys.stderr)
        return 1
    out = sys.stdout.buffer
    if gfa:
        for recs, g in zip(records, graphs):
            out.write(g.to_gfa([name for name, _, _ in recs], include_consensus=a.gfa_consensus))
    elif cons is not None:
        for c in cons:
            out.write(b">Consensus LN:i:%d\n%s\n" % (len(c), c))
    elif a.r == 0:
        for m in msa:
            cv = b"".join(b",%d" % x for x in m.coverage)
            out.write(b">Consensus LN:i:%d CV:B:I%s\n%s\n" % (len(m.consensus), cv, m.consensus))
    else:
        for recs, m in zip(records, msa):
            for row, mb in zip(m.rows, m.members):
                name = b"Consensus" if mb == CONSENSUS_ROW else _bytes(recs[mb][0], "record name")
                out.write(b">%s\n%s\n" % (name, row))
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
