"""ctypes binding of the C ABI declared in include/vechat_hip.h.

This is plumbing: the product is libvechat_hip.so (HIP kernels + C ABI).  There is deliberately
no CPU fallback here -- if the HIP library is missing or no gfx950 device is visible the calls
raise.  libvechat_host.so (host helpers only, no device code) serves the CPU-only tests.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

VC_WIN_OK, VC_WIN_UNPOLISHED, VC_WIN_OVERFLOW, VC_WIN_UNSUPPORTED, VC_WIN_INVALID = range(5)
VC_OK, VC_ERR_ARG, VC_ERR_HIP, VC_ERR_NO_DEVICE, VC_ERR_STATE, VC_ERR_CAPACITY = 0, -1, -2, -3, -4, -5


class VcParams(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32),
        ("sw_match", C.c_int32), ("sw_mismatch", C.c_int32), ("sw_gap", C.c_int32),
        ("min_confidence", C.c_double), ("min_support", C.c_double),
        ("num_prune", C.c_uint32),
        ("mode", C.c_int32), ("trim", C.c_int32), ("window_type", C.c_int32),
        ("max_nodes", C.c_uint32), ("max_edges", C.c_uint32), ("chunk_windows", C.c_uint32),
        ("scratch_bytes", C.c_uint64),
        ("profile", C.c_int32),
        ("n_streams", C.c_uint32),
    ]


class VcBatch(C.Structure):
    _fields_ = [
        ("n_windows", C.c_uint32),
        ("win_seq_off", C.POINTER(C.c_uint32)),
        ("seq_off", C.POINTER(C.c_uint64)),
        ("seq_begin", C.POINTER(C.c_uint32)),
        ("seq_end", C.POINTER(C.c_uint32)),
        ("seq_has_qual", C.POINTER(C.c_uint8)),
        ("bases", C.POINTER(C.c_uint8)),
        ("quals", C.POINTER(C.c_uint8)),
        ("win_fasta", C.POINTER(C.c_uint8)),
    ]


class VcResult(C.Structure):
    _fields_ = [
        ("cons_off", C.POINTER(C.c_uint64)),
        ("cons", C.POINTER(C.c_uint8)),
        ("cons_cap", C.c_uint64),
        ("status", C.POINTER(C.c_uint8)),
    ]


class VcPoaParams(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("algorithm", C.c_int32),
        ("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32),
    ]


class VcPoaGapParams(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("algorithm", C.c_int32),
        ("match", C.c_int32), ("mismatch", C.c_int32),
        ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("gap_open2", C.c_int32), ("gap_extend2", C.c_int32),
    ]


VC_POA_MSA, VC_POA_MSA_CONSENSUS, VC_POA_COVERAGE = 1, 2, 4
VC_POA_ROW_CONSENSUS = 0xFFFFFFFF


class VcPoaMsaOut(C.Structure):
    """vc_poa_msa_out: flags in, the rest out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("flags", C.c_uint32), ("n_groups", C.c_uint32),
        ("n_rows", C.POINTER(C.c_uint32)), ("row_size", C.POINTER(C.c_uint32)),
        ("row_off", C.POINTER(C.c_uint64)), ("member_off", C.POINTER(C.c_uint64)),
        ("row_member", C.POINTER(C.c_uint32)),
        ("rows", C.POINTER(C.c_uint8)), ("rows_bytes", C.c_uint64),
        ("coverage", C.POINTER(C.c_uint32)),
    ]


class VcPoaStrandOut(C.Structure):
    """vc_poa_strand_out: caller-owned arrays, one entry per sequence of the batch; score / score_rev may be NULL"""
    _fields_ = [("reversed", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32)), ("score_rev", C.POINTER(C.c_int32))]


class VcPoaGraphOut(C.Structure):
    """vc_poa_graph_out: everything out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("n_groups", C.c_uint32),
        ("n_nodes", C.POINTER(C.c_uint32)), ("node_off", C.POINTER(C.c_uint64)), ("node_base", C.POINTER(C.c_uint8)),
        ("node_cons_pos", C.POINTER(C.c_int32)), ("rank_to_node", C.POINTER(C.c_uint32)),
        ("out_off", C.POINTER(C.c_uint64)), ("edge_head", C.POINTER(C.c_uint32)), ("edge_weight", C.POINTER(C.c_int64)),
        ("aligned_off", C.POINTER(C.c_uint64)), ("aligned_a", C.POINTER(C.c_uint32)), ("aligned_b", C.POINTER(C.c_uint32)),
        ("path_first", C.POINTER(C.c_uint64)), ("path_member", C.POINTER(C.c_uint32)), ("path_reversed", C.POINTER(C.c_uint8)),
        ("path_off", C.POINTER(C.c_uint64)), ("path_node", C.POINTER(C.c_uint32)),
        ("cons_node", C.POINTER(C.c_uint32)),
        ("bytes", C.c_uint64),
    ]


VC_POA_ALIGN_PAIRS, VC_POA_ALIGN_STRANDS = 1, 2


class VcPoaAlignOut(C.Structure):
    """vc_poa_align_out: flags in, the rest out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("flags", C.c_uint32), ("n_queries", C.c_uint64),
        ("status", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32)), ("score_rev", C.POINTER(C.c_int32)),
        ("reversed", C.POINTER(C.c_uint8)),
        ("pair_off", C.POINTER(C.c_uint64)), ("pair_node", C.POINTER(C.c_int32)), ("pair_pos", C.POINTER(C.c_int32)),
        ("bytes", C.c_uint64),
    ]


VC_POA_ASSIGN_STRANDS, VC_POA_ASSIGN_SCORES = 1, 2


class VcPoaAssignOut(C.Structure):
    """vc_poa_assign_out: flags in, the rest out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("flags", C.c_uint32), ("n_queries", C.c_uint64), ("n_groups", C.c_uint32),
        ("status", C.POINTER(C.c_uint8)),
        ("best_group", C.POINTER(C.c_int32)), ("best_score", C.POINTER(C.c_int32)),
        ("second_group", C.POINTER(C.c_int32)), ("second_score", C.POINTER(C.c_int32)),
        ("reversed", C.POINTER(C.c_uint8)),
        ("scores", C.POINTER(C.c_int32)), ("pair_status", C.POINTER(C.c_uint8)),
        ("bytes", C.c_uint64),
    ]


class VcPoaStateOut(C.Structure):
    """vc_poa_state_out: every node's aligned list, owned by the library as vc_poa_graph_out is"""
    _fields_ = [("al_off", C.POINTER(C.c_uint64)), ("al_node", C.POINTER(C.c_uint32)), ("bytes", C.c_uint64)]


class VcPoaGraphIn(C.Structure):
    """vc_poa_graph_in: caller-owned arrays of stored graphs, laid out as vc_poa_graph_out and vc_poa_state_out are"""
    _fields_ = [
        ("n_groups", C.c_uint32), ("n_members", C.POINTER(C.c_uint32)),
        ("n_nodes", C.POINTER(C.c_uint32)), ("node_off", C.POINTER(C.c_uint64)), ("node_base", C.POINTER(C.c_uint8)),
        ("rank_to_node", C.POINTER(C.c_uint32)),
        ("out_off", C.POINTER(C.c_uint64)), ("edge_head", C.POINTER(C.c_uint32)), ("edge_weight", C.POINTER(C.c_int64)),
        ("al_off", C.POINTER(C.c_uint64)), ("al_node", C.POINTER(C.c_uint32)),
        ("path_first", C.POINTER(C.c_uint64)), ("path_member", C.POINTER(C.c_uint32)), ("path_reversed", C.POINTER(C.c_uint8)),
        ("path_off", C.POINTER(C.c_uint64)), ("path_node", C.POINTER(C.c_uint32)),
    ]


VC_POA_SPAN_NONE = 0xFFFFFFFF


class VcPoaSpanIn(C.Structure):
    """vc_poa_span_in: caller-owned, one (begin, end) per sequence of the batch; VC_POA_SPAN_NONE in both: the whole graph"""
    _fields_ = [("begin", C.POINTER(C.c_uint32)), ("end", C.POINTER(C.c_uint32))]


class VcPoaWeightIn(C.Structure):
    """vc_poa_weight_in: caller-owned; mode per sequence of the batch (0 as the batch says, 1 seq_weight, 2 base_weight at seq_off's offsets)"""
    _fields_ = [("mode", C.POINTER(C.c_uint8)), ("seq_weight", C.POINTER(C.c_uint32)), ("base_weight", C.POINTER(C.c_uint32))]


class VcPoaProfileOut(C.Structure):
    """vc_poa_profile_out: library-owned; per group its codes and a block of (n_codes + 1) rows x consensus length counts, gaps last"""
    _fields_ = [("n_groups", C.c_uint32), ("n_codes", C.POINTER(C.c_uint32)), ("code_off", C.POINTER(C.c_uint64)),
                ("codes", C.POINTER(C.c_uint8)), ("prof_off", C.POINTER(C.c_uint64)), ("counts", C.POINTER(C.c_uint32))]


VC_POA_HAP_MAX, VC_POA_HAP_INDELS, VC_POA_HAP_NONE = 8, 1, 0xFF


class VcPoaHapParams(C.Structure):
    """vc_poa_hap_params: the haplotype rule's parameters (defaults 2 / 2 / 250 / 4 / 0, vc_poa_hap_default_params)"""
    _fields_ = [("max_haplotypes", C.c_uint32), ("min_reads", C.c_uint32), ("min_permille", C.c_uint32), ("rounds", C.c_uint32),
                ("flags", C.c_uint32)]


class VcPoaHapOut(C.Structure):
    """vc_poa_hap_out: everything out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("n_groups", C.c_uint32),
        ("n_haps", C.POINTER(C.c_uint32)), ("hap_first", C.POINTER(C.c_uint64)), ("hap_size", C.POINTER(C.c_uint32)),
        ("cons_off", C.POINTER(C.c_uint64)), ("cons", C.POINTER(C.c_uint8)), ("hap_of", C.POINTER(C.c_uint8)),
        ("site_off", C.POINTER(C.c_uint64)), ("site_col", C.POINTER(C.c_uint32)),
        ("site_major", C.POINTER(C.c_uint8)), ("site_minor", C.POINTER(C.c_uint8)),
        ("site_n_major", C.POINTER(C.c_uint32)), ("site_n_minor", C.POINTER(C.c_uint32)),
        ("bytes", C.c_uint64),
    ]


class VcPoaPruneParams(C.Structure):
    """vc_poa_prune_params: the thresholds and rounds of vc_poa_run_correct (the reference's defaults: 0.22 / 0.19 / 3)"""
    _fields_ = [("min_confidence", C.c_double), ("min_support", C.c_double), ("num_prune", C.c_uint32)]


class VcPoaCorrectOut(C.Structure):
    """vc_poa_correct_out: everything out and owned by the library until its next vc_poa_* / vc_large_* call"""
    _fields_ = [
        ("n_seqs", C.c_uint64),
        ("status", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32)),
        ("corr_off", C.POINTER(C.c_uint64)), ("corr", C.POINTER(C.c_uint8)),
        ("bytes", C.c_uint64),
    ]


class VcStats(C.Structure):
    _fields_ = [
        ("cells", C.c_uint64), ("alignments", C.c_uint64), ("dp_rows", C.c_uint64),
        ("far_row_reads", C.c_uint64), ("trace_steps", C.c_uint64), ("trace_spec", C.c_uint64), ("trace_rounds", C.c_uint64),
        ("n_classes", C.c_uint32),
        ("ms", C.c_double * 16),
        ("launches", C.c_uint64 * 16),
        ("names", (C.c_char * 24) * 16),
        ("max_nodes", C.c_uint32), ("max_edges", C.c_uint32), ("chunk_windows", C.c_uint32), ("n_streams", C.c_uint32),
        ("busy_ms", C.c_double * 16),
        ("band_redo", C.c_uint64), ("device_bytes", C.c_uint64),
        ("fwd_shader_cycles", C.c_uint64), ("fwd_wall_ticks", C.c_uint64),
    ]


class VcOverlapRec(C.Structure):
    _fields_ = [
        ("q_name", C.c_void_p), ("q_name_len", C.c_uint32), ("t_name", C.c_void_p), ("t_name_len", C.c_uint32),
        ("by_index", C.c_uint8), ("q_index", C.c_uint32), ("t_index", C.c_uint32), ("strand", C.c_uint8),
        ("q_begin", C.c_uint32), ("q_end", C.c_uint32), ("q_length", C.c_uint32), ("t_begin", C.c_uint32), ("t_end", C.c_uint32),
        ("length", C.c_uint32), ("error", C.c_double), ("cigar", C.c_char_p), ("dropped", C.c_uint8),
    ]


class VcSynthCfg(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("backbone_len", C.c_uint32), ("n_layers", C.c_uint32),
        ("error_rate", C.c_double),
        ("frac_ins", C.c_double), ("frac_del", C.c_double), ("frac_sub", C.c_double),
        ("frac_partial", C.c_double),
        ("fastq", C.c_int32), ("backbone_fastq", C.c_int32),
        ("n_haplotypes", C.c_int32),
        ("snp_rate", C.c_double),
    ]


class VcAlignBatch(C.Structure):
    _fields_ = [("n", C.c_uint32), ("q_off", C.POINTER(C.c_uint64)), ("q", C.POINTER(C.c_uint8)),
                ("t_off", C.POINTER(C.c_uint64)), ("t", C.POINTER(C.c_uint8))]


class VcOverlapSeqs(C.Structure):
    _fields_ = [("n", C.c_uint64), ("off", C.POINTER(C.c_uint64)), ("bases", C.POINTER(C.c_uint8))]


class VcOverlapParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("device", "k", "w", "max_occ", "max_gap", "bandwidth", "lookback", "min_chain_score", "min_anchors",
                                         "min_overlap", "drop_internal", "same_set")]


class VcOverlapOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("q_id", C.POINTER(C.c_uint32)), ("t_id", C.POINTER(C.c_uint32)), ("strand", C.POINTER(C.c_uint8)),
                ("q_begin", C.POINTER(C.c_uint32)), ("q_end", C.POINTER(C.c_uint32)), ("t_begin", C.POINTER(C.c_uint32)),
                ("t_end", C.POINTER(C.c_uint32)), ("n_anchors", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_int32)),
                ("matches", C.POINTER(C.c_uint32)), ("block", C.POINTER(C.c_uint32)),
                ("n_minimizers", C.c_uint64), ("n_anchors_total", C.c_uint64), ("n_keys_total", C.c_uint64)]


class VcOverlapSketchOut(C.Structure):
    _fields_ = [("n", C.c_uint64), ("hash", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
                ("strand", C.POINTER(C.c_uint8))]


class VcScrubParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("device", "coverage", "max_bad_permille", "min_piece")]


class VcScrubIn(C.Structure):
    _fields_ = [("n", C.c_uint64), ("len", C.POINTER(C.c_uint32)), ("m", C.c_uint64), ("read", C.POINTER(C.c_uint32)),
                ("begin", C.POINTER(C.c_uint32)), ("end", C.POINTER(C.c_uint32)), ("off", C.POINTER(C.c_uint64)),
                ("bases", C.POINTER(C.c_uint8)), ("quals", C.POINTER(C.c_uint8))]


class VcScrubOut(C.Structure):
    _fields_ = [("n_regions", C.c_uint64), ("reg_read", C.POINTER(C.c_uint32)), ("reg_begin", C.POINTER(C.c_uint32)),
                ("reg_end", C.POINTER(C.c_uint32)), ("reg_off", C.POINTER(C.c_uint64)), ("klass", C.POINTER(C.c_uint8)),
                ("bad_total", C.POINTER(C.c_uint32)), ("n_pieces", C.c_uint64), ("pc_read", C.POINTER(C.c_uint32)),
                ("pc_begin", C.POINTER(C.c_uint32)), ("pc_end", C.POINTER(C.c_uint32)), ("pc_off", C.POINTER(C.c_uint64)),
                ("pc_bases", C.POINTER(C.c_uint8)), ("pc_quals", C.POINTER(C.c_uint8)),
                ("n_intervals", C.c_uint64), ("n_events", C.c_uint64), ("n_segments", C.c_uint64)]


class VcClusterParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("device", "min_overlap", "min_cover_permille", "cover_both", "min_identity_permille", "min_size",
                                         "by_size", "longest_first")]


CLUSTER_RECORD_FIELDS = (("q_id", C.c_uint32), ("t_id", C.c_uint32), ("strand", C.c_uint8), ("q_begin", C.c_uint32), ("q_end", C.c_uint32),
                         ("t_begin", C.c_uint32), ("t_end", C.c_uint32), ("matches", C.c_uint32), ("block", C.c_uint32))


class VcClusterIn(C.Structure):
    _fields_ = [("n", C.c_uint64), ("len", C.POINTER(C.c_uint32)), ("m", C.c_uint64)] + [(f, C.POINTER(t)) for f, t in CLUSTER_RECORD_FIELDS]


class VcClusterOut(C.Structure):
    _fields_ = [("n_clusters", C.c_uint64), ("cl_off", C.POINTER(C.c_uint64)), ("members", C.POINTER(C.c_uint32)),
                ("cl_root", C.POINTER(C.c_uint32)), ("cl_twisted", C.POINTER(C.c_uint8)), ("cluster", C.POINTER(C.c_uint32)),
                ("strand", C.POINTER(C.c_uint8)), ("n_links", C.c_uint64), ("n_rounds", C.c_uint64), ("n_components", C.c_uint64)]


class VcDemuxParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("device", "window", "max_err_permille", "min_margin", "trim", "flags")]


class VcDemuxIn(C.Structure):
    _fields_ = [("n", C.c_uint64), ("off", C.POINTER(C.c_uint64)), ("bases", C.POINTER(C.c_uint8)), ("quals", C.POINTER(C.c_uint8)),
                ("n_patterns", C.c_uint64), ("pat_off", C.POINTER(C.c_uint64)), ("pat_bases", C.POINTER(C.c_uint8)),
                ("label", C.POINTER(C.c_uint32)), ("side", C.POINTER(C.c_uint8))]


class VcDemuxOut(C.Structure):
    _fields_ = [("v_pat", C.POINTER(C.c_uint32)), ("v_dist", C.POINTER(C.c_uint8)), ("v_start", C.POINTER(C.c_uint32)),
                ("v_end", C.POINTER(C.c_uint32)), ("v_second", C.POINTER(C.c_uint8)), ("klass", C.POINTER(C.c_uint8)),
                ("label", C.POINTER(C.c_uint32)), ("flip", C.POINTER(C.c_uint8)), ("begin", C.POINTER(C.c_uint32)),
                ("end", C.POINTER(C.c_uint32)), ("piece_off", C.POINTER(C.c_uint64)), ("pc_bases", C.POINTER(C.c_uint8)),
                ("pc_quals", C.POINTER(C.c_uint8)), ("n_labels", C.c_uint64), ("grp_off", C.POINTER(C.c_uint64)),
                ("grp_reads", C.POINTER(C.c_uint32)), ("all_dist", C.POINTER(C.c_uint8)), ("all_end", C.POINTER(C.c_uint32)),
                ("n_reads", C.c_uint64), ("n_triples", C.c_uint64), ("n_budget_pieces", C.c_uint64), ("n_accepted", C.c_uint64)]


def default_params(**kw):
    """Defaults the Python driver ends up with (scripts/vechat:70-72: -d 0.2 -s 0.2; main.cpp:46-61)."""
    p = VcParams(device=0, match=3, mismatch=-5, gap=-4, sw_match=3, sw_mismatch=-5, sw_gap=-4,
                 min_confidence=0.2, min_support=0.2, num_prune=3, mode=0, trim=1, window_type=1,
                 max_nodes=0, max_edges=0, chunk_windows=0, scratch_bytes=0, profile=0, n_streams=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _take(ptr, n, dtype):
    """a copy of n entries of a library-owned array"""
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)


def pack(seqs):
    """[bytes] -> (VcOverlapSeqs, the arrays that must outlive it)"""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    bases = np.frombuffer(b"".join(bytes(s) for s in seqs) + b"\0", np.uint8).copy()
    return VcOverlapSeqs(len(seqs), _ptr(off, C.c_uint64), _ptr(bases, C.c_uint8)), (off, bases)


def params_from_defaults(struct, c_default, fields, what, kw):
    """a parameter struct as its C default function fills it, then kw: the one body of overlap / scrub / cluster.default_params"""
    p = struct()
    c_default(C.byref(p))
    for name, v in kw.items():
        if name != "device" and name not in fields:
            raise TypeError(f"unknown {what} parameter {name!r}")
        setattr(p, name, int(v))
    return p


class Batch:
    """A packed window batch held in numpy arrays (layout of struct vc_batch)."""

    def __init__(self, win_seq_off, seq_off, seq_begin, seq_end, seq_has_qual, bases, quals,
                 win_fasta, seq_orig=None):
        self.win_seq_off = np.ascontiguousarray(win_seq_off, dtype=np.uint32)
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        self.seq_begin = np.ascontiguousarray(seq_begin, dtype=np.uint32)
        self.seq_end = np.ascontiguousarray(seq_end, dtype=np.uint32)
        self.seq_has_qual = np.ascontiguousarray(seq_has_qual, dtype=np.uint8)
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.quals = np.ascontiguousarray(quals, dtype=np.uint8)
        self.win_fasta = np.ascontiguousarray(win_fasta, dtype=np.uint8)
        self.seq_orig = None if seq_orig is None else np.ascontiguousarray(seq_orig, dtype=np.uint32)
        if self.bases.size == 0:
            self.bases = np.zeros(1, np.uint8)
            self.quals = np.zeros(1, np.uint8)

    @property
    def n_windows(self):
        return int(self.win_fasta.size)

    @property
    def n_seqs(self):
        return int(self.seq_begin.size)

    def as_struct(self, cls=VcBatch):
        return cls(self.n_windows, _ptr(self.win_seq_off, C.c_uint32), _ptr(self.seq_off, C.c_uint64),
                   _ptr(self.seq_begin, C.c_uint32), _ptr(self.seq_end, C.c_uint32),
                   _ptr(self.seq_has_qual, C.c_uint8), _ptr(self.bases, C.c_uint8),
                   _ptr(self.quals, C.c_uint8), _ptr(self.win_fasta, C.c_uint8))

    def window(self, w):
        """(seqs, quals|None, begins, ends) of window w in stored (rank) order, as bytes."""
        s0, s1 = int(self.win_seq_off[w]), int(self.win_seq_off[w + 1])
        seqs, quals, b, e = [], [], [], []
        for s in range(s0, s1):
            o0, o1 = int(self.seq_off[s]), int(self.seq_off[s + 1])
            seqs.append(self.bases[o0:o1].tobytes())
            quals.append(self.quals[o0:o1].tobytes() if self.seq_has_qual[s] else None)
            b.append(int(self.seq_begin[s]))
            e.append(int(self.seq_end[s]))
        return seqs, quals, b, e

    def slice(self, lo, hi):
        """Windows [lo, hi) as a new Batch (contiguous range: offsets rebased, no per-window work)."""
        s0, s1 = int(self.win_seq_off[lo]), int(self.win_seq_off[hi])
        b0, b1 = int(self.seq_off[s0]), int(self.seq_off[s1])
        return Batch(self.win_seq_off[lo:hi + 1] - np.uint32(s0), self.seq_off[s0:s1 + 1] - np.uint64(b0),
                     self.seq_begin[s0:s1], self.seq_end[s0:s1], self.seq_has_qual[s0:s1], self.bases[b0:b1],
                     self.quals[b0:b1], self.win_fasta[lo:hi], None if self.seq_orig is None else self.seq_orig[s0:s1])

    def select(self, idx):
        """A new Batch holding windows idx (in that order)."""
        return Batch.from_windows([self.window(w) for w in idx], [int(self.win_fasta[w]) for w in idx],
                                  presorted=True)

    @staticmethod
    def from_windows(windows, fasta_flags, presorted=False, host=None):
        """windows: list of (seqs, quals|None, begins, ends); sequence 0 is the backbone.
        Unless presorted, layers are put into the reference's rank order (vc_rank_layers)."""
        wso, so, sb, se, hq, bases, quals, orig = [0], [0], [], [], [], [], [], []
        for seqs, qs, b, e in windows:
            n = len(seqs)
            order = list(range(n))
            if not presorted:
                host = host or load_host()
                rk = (C.c_uint32 * n)()
                host.vc_rank_layers((C.c_uint32 * n)(*b), n, rk)
                order = list(rk)
            for i in order:
                bases.append(seqs[i])
                quals.append(qs[i] if qs[i] is not None else b"!" * len(seqs[i]))
                so.append(so[-1] + len(seqs[i]))
                sb.append(b[i]); se.append(e[i]); hq.append(0 if qs[i] is None else 1)
                orig.append(i)
            wso.append(len(sb))
        return Batch(np.array(wso), np.array(so, dtype=np.uint64), np.array(sb), np.array(se), np.array(hq),
                     np.frombuffer(b"".join(bases), dtype=np.uint8), np.frombuffer(b"".join(quals), dtype=np.uint8),
                     np.array(fasta_flags), np.array(orig))


_P = C.POINTER
_vp, _str, _int, _u32, _u64, _f64 = C.c_void_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
_u8p, _u32p, _i32p, _u64p = _P(C.c_uint8), _P(C.c_uint32), _P(C.c_int32), _P(C.c_uint64)
_batch, _result, _params, _gap = _P(VcBatch), _P(VcResult), _P(VcParams), _P(VcPoaGapParams)
_msa, _strand, _graph, _graph_in, _align = _P(VcPoaMsaOut), _P(VcPoaStrandOut), _P(VcPoaGraphOut), _P(VcPoaGraphIn), _P(VcPoaAlignOut)
_oseqs = _P(VcOverlapSeqs)

# Every entry of include/vechat_hip.h that Python calls: name -> (restype, argtypes), in the header's order.  A new entry point is one
# row here (and one structure above if it has one); tests/test_capi_table.py holds the table against the header's prototypes.
SIGNATURES = {
    "vc_create": (_int, [_P(_vp), _params]),
    "vc_destroy": (None, [_vp]),
    "vc_last_error": (_str, [_vp]),
    "vc_submit": (_int, [_vp, _batch]),
    "vc_run": (_int, [_vp]),
    "vc_sync": (_int, [_vp]),
    "vc_result_windows": (_int, [_vp, _u32p]),
    "vc_result_size": (_int, [_vp, _u64p]),
    "vc_collect": (_int, [_vp, _result]),
    "vc_collect_device": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "vc_get_stats": (_int, [_vp, _P(VcStats)]),
    "vc_debug_errinfo": (_int, [_vp, _u32p]),
    "vc_debug_stop_after": (_int, [_vp, _u32, _u32]),
    "vc_debug_stage_digest": (_int, [_vp, _u32, _int, _u64p]),
    "vc_debug_rows": (_int, [_vp, _u32, _u32p, _u32, _u32p]),
    "vc_stream": (_vp, [_vp]),
    "vc_set_profile": (_int, [_vp, _int]),
    "vc_has_experiments": (_int, []),
    "vc_reserve": (_int, [_vp, _u64]),
    "vc_set_polish_params": (_int, [_vp, _params]),
    "vc_release": (_int, [_vp]),
    "vc_set_window_type": (_int, [_vp, _int]),
    # host helpers: from here to vc_io_load the rows are HOST_ENTRIES, all that libvechat_host.so has
    "vc_rank_layers": (None, [_u32p, _u32, _u32p]),
    "vc_backbone_is_fasta": (_int, [_str, _u32]),
    "vc_weight_lut": (None, [_u32p]),
    "vc_synth_generate": (_vp, [_P(VcSynthCfg), _u64, _u32, _u32]),
    "vc_synth_batch": (None, [_vp, _batch]),
    "vc_synth_n_seqs": (_u64, [_vp]),
    "vc_synth_orig_index": (_u32p, [_vp]),
    "vc_synth_n_bytes": (_u64, [_vp]),
    "vc_synth_free": (None, [_vp]),
    "vc_wb_create": (_vp, [_u32, _f64]),
    "vc_wb_destroy": (None, [_vp]),
    "vc_wb_last_error": (_str, [_vp]),
    "vc_wb_add_sequence": (_int, [_vp, _str, _str, _u32, _str]),
    "vc_wb_set_targets": (_int, [_vp, _u32]),
    "vc_wb_add_overlap": (_int, [_vp, _u32, _u32, _int, _u32, _u32, _u32, _u32, _u32, _str]),
    "vc_wb_n_breaking_points": (_u32, [_vp, _u32]),
    "vc_wb_breaking_points": (None, [_vp, _u32, _u32p, _u32p]),
    "vc_wb_build": (_int, [_vp, _batch]),
    "vc_wb_build_begin": (_int, [_vp, _batch]),
    "vc_wb_build_fill": (_int, [_vp, _u32, _u32]),
    "vc_wb_seq_orig": (_u32p, [_vp]),
    "vc_wb_n_windows": (_u32, [_vp]),
    "vc_wb_window_target": (_u32, [_vp, _u32]),
    "vc_wb_window_rank": (_u32, [_vp, _u32]),
    "vc_wb_window_ids": (None, [_vp, _u32p, _u32p]),
    "vc_wb_stitch": (_int, [_vp, _result, _int, _int]),
    "vc_wb_n_polished": (_u32, [_vp]),
    "vc_wb_polished_name": (_str, [_vp, _u32]),
    "vc_wb_polished_data": (_P(C.c_char), [_vp, _u32, _u64p]),
    "vc_io_read_sequences": (_vp, [_str, _str, _int]),
    "vc_seqset_free": (None, [_vp]),
    "vc_seqset_error": (_str, [_vp]),
    "vc_seqset_size": (_u64, [_vp]),
    "vc_seqset_name_off": (_u64p, [_vp]),
    "vc_seqset_names": (_vp, [_vp]),
    "vc_seqset_data_off": (_u64p, [_vp]),
    "vc_seqset_data": (_vp, [_vp]),
    "vc_seqset_qual": (_vp, [_vp]),
    "vc_seqset_has_qual": (_u8p, [_vp]),
    "vc_seqset_lengths": (_u64p, [_vp]),
    "vc_io_read_overlaps": (_vp, [_str]),
    "vc_ovlset_free": (None, [_vp]),
    "vc_ovlset_error": (_str, [_vp]),
    "vc_ovlset_size": (_u64, [_vp]),
    "vc_ovlset_get": (_int, [_vp, _u64, _P(VcOverlapRec)]),
    "vc_ovlset_set_cigar": (_int, [_vp, _u64, _str]),
    "vc_io_target_cost": (_int, [_vp, _vp, _P(_f64)]),
    "vc_io_rank_names": (_vp, [_vp, _vp, _vp, _u64, _u64, _u64p]),
    "vc_io_free": (None, [_vp]),
    "vc_io_load": (C.c_int64, [_vp, _vp, _vp, _vp, _f64, _int, _P(_int), _str, _u64]),
    "vc_align": (_int, [_int, _P(VcAlignBatch), _str, _u64, _u64p, _i32p]),
    "vc_align_last_error": (_str, []),
    "vc_align_release": (None, []),
    "vc_large_run": (_int, [_params, _batch, _result]),
    "vc_large_last_error": (_str, []),
    "vc_large_release": (None, []),
    "vc_poa_run": (_int, [_P(VcPoaParams), _batch, _result]),
    "vc_poa_last_error": (_str, []),
    "vc_poa_run_gaps": (_int, [_gap, _batch, _result]),
    "vc_poa_run_msa": (_int, [_gap, _batch, _result, _msa]),
    "vc_poa_run_strand": (_int, [_gap, _batch, _result, _msa, _strand]),
    "vc_poa_run_graph": (_int, [_gap, _batch, _result, _msa, _strand, _graph]),
    "vc_poa_run_align": (_int, [_gap, _batch, _result, _strand, _graph, _batch, _align]),
    "vc_poa_run_correct": (_int, [_batch, _gap, _P(VcPoaPruneParams), _result, _P(VcPoaCorrectOut)]),
    "vc_poa_run_from": (_int, [_gap, _graph_in, _batch, _result, _msa, _strand, _graph, _P(VcPoaStateOut), _batch, _align]),
    "vc_poa_run_assign": (_int, [_gap, _graph_in, _batch, _result, _batch, _P(VcPoaAssignOut)]),
    "vc_poa_run_spans": (_int, [_gap, _P(VcPoaSpanIn), _batch, _result, _msa, _strand, _graph]),
    "vc_poa_run_weighted": (_int, [_gap, _P(VcPoaWeightIn), _batch, _result, _msa, _strand, _graph, _P(VcPoaProfileOut)]),
    "vc_poa_hap_default_params": (None, [_P(VcPoaHapParams)]),
    "vc_poa_run_haplotypes": (_int, [_gap, _P(VcPoaHapParams), _batch, _result, _P(VcPoaHapOut)]),
    "vc_overlap_default_params": (None, [_P(VcOverlapParams)]),
    "vc_overlap": (_int, [_P(VcOverlapParams), _oseqs, _oseqs, _P(VcOverlapOut)]),
    "vc_overlap_sketch": (_int, [C.c_int32, C.c_int32, C.c_int32, _oseqs, _P(VcOverlapSketchOut)]),
    "vc_overlap_last_error": (_str, []),
    "vc_overlap_release": (None, []),
    "vc_scrub_default_params": (None, [_P(VcScrubParams)]),
    "vc_scrub": (_int, [_P(VcScrubParams), _P(VcScrubIn), _P(VcScrubOut)]),
    "vc_scrub_last_error": (_str, []),
    "vc_scrub_release": (None, []),
    "vc_cluster_default_params": (None, [_P(VcClusterParams)]),
    "vc_cluster": (_int, [_P(VcClusterParams), _P(VcClusterIn), _P(VcClusterOut)]),
    "vc_cluster_last_error": (_str, []),
    "vc_cluster_release": (None, []),
    "vc_demux_default_params": (None, [_P(VcDemuxParams)]),
    "vc_demux": (_int, [_P(VcDemuxParams), _P(VcDemuxIn), _P(VcDemuxOut)]),
    "vc_demux_last_error": (_str, []),
    "vc_demux_release": (None, []),
}
_names = list(SIGNATURES)
HOST_ENTRIES = tuple(_names[_names.index("vc_rank_layers"):_names.index("vc_io_load") + 1])


def bind(lib, names=None, optional=False):
    """Sets restype and argtypes of the named entries of SIGNATURES (None: all of them) on a loaded library and returns it.  A symbol
    the library lacks is an AttributeError naming it, or with optional=True is passed over: the library is older than this module."""
    for name in SIGNATURES if names is None else names:
        if optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


_host = None
_hip = None


def load_host():
    """Host helpers only (rank sort, fasta flag, LUT, synthetic generator)."""
    global _host
    if _host is None:
        path = os.path.join(LIB_DIR, "libvechat_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _host = bind(C.CDLL(path), HOST_ENTRIES)
    return _host


def load_hip():
    """The product library.  Raises if it has not been built; never falls back to CPU code.  Only a library named by VECHAT_HIP_LIB
    (development A/B builds, the parent commit's library beside which tools/gpu_poa_rate.py measures) may predate an entry point:
    poa._entry says so when such an entry is asked for."""
    global _hip
    if _hip is None:
        override = os.environ.get("VECHAT_HIP_LIB")
        path = override or os.path.join(LIB_DIR, "libvechat_hip.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is required (no CPU fallback); "
                               "run `python -c 'import __graft_entry__ as g; g.build()'`")
        _hip = bind(C.CDLL(path), optional=bool(override))
    return _hip


PACBIO = dict(error_rate=0.15, frac_ins=0.40, frac_del=0.30, frac_sub=0.30)
ONT = dict(error_rate=0.10, frac_ins=0.25, frac_del=0.45, frac_sub=0.30)


def synth_cfg(seed, backbone_len, n_layers, profile=PACBIO, frac_partial=0.0, fastq=1,
              backbone_fastq=1, n_haplotypes=1, snp_rate=0.01):
    return VcSynthCfg(seed=seed, backbone_len=backbone_len, n_layers=n_layers,
                      error_rate=profile["error_rate"], frac_ins=profile["frac_ins"],
                      frac_del=profile["frac_del"], frac_sub=profile["frac_sub"],
                      frac_partial=frac_partial, fastq=fastq, backbone_fastq=backbone_fastq,
                      n_haplotypes=n_haplotypes, snp_rate=snp_rate)


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota, shared out over the ranks
    of a one-process-per-GPU launch on this node (LOCAL_WORLD_SIZE): eight ranks must not start eight full-size pools."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    try:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    except ValueError:
        local_world = 1
    return max(1, n // max(1, local_world))


def synth_batch(cfg, first, n, n_threads=0, lib=None):
    """Generate windows [first, first+n) of the synthetic stream as a Batch (rank-ordered layers)."""
    lib = lib or load_host()
    n_threads = n_threads or min(usable_cores(), 32)
    h = lib.vc_synth_generate(C.byref(cfg), first, n, n_threads)
    if not h:
        raise RuntimeError("vc_synth_generate failed")
    try:
        vb = VcBatch()
        lib.vc_synth_batch(h, C.byref(vb))
        ns = lib.vc_synth_n_seqs(h)
        nb = lib.vc_synth_n_bytes(h)
        arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(int(k),)).astype(dt, copy=True)
        return Batch(arr(vb.win_seq_off, n + 1, np.uint32), arr(vb.seq_off, ns + 1, np.uint64),
                     arr(vb.seq_begin, ns, np.uint32), arr(vb.seq_end, ns, np.uint32),
                     arr(vb.seq_has_qual, ns, np.uint8), arr(vb.bases, max(nb, 1), np.uint8)[:nb] if nb else np.zeros(0, np.uint8),
                     arr(vb.quals, max(nb, 1), np.uint8)[:nb] if nb else np.zeros(0, np.uint8),
                     arr(vb.win_fasta, n, np.uint8), arr(lib.vc_synth_orig_index(h), ns, np.uint32))
    finally:
        lib.vc_synth_free(h)
