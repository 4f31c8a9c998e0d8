// The large-graph path: the whole per-window algorithm on the device without the fast path's limits.
//
// The fast path (vc_api.hip) holds 16-bit node ids, LDS graph images and 16-bit adjacency offsets, so a window's graph stops at
// 59 968 nodes / 32 000 edges and a window with a longer layer stops at k_addaln's LDS notes; such windows come back
// VC_WIN_OVERFLOW.  vc_large_run computes them here: every id is 32 bits, every score int32 (int64 inside the horizontal scan),
// every table lives in HBM and is sized from what the window needs; a window whose tables fill is run again with larger ones.
// Slow by design: correctness counts here, not speed.
//
// Three schedules (LArgs::mode), each a window / group per lane of the kernels below:
//   0 haplotype overload (window.cpp:176-428): rank-ordered layers, subgraphs of partial-span layers, prune rounds, the final
//     local alignment of the backbone -- vc_large_run;
//   1 racon-linear overload (window.cpp:74-170): the same build, then heaviest bundle + coverage + TGS trim -- vc_large_run;
//   2 POA group, vc_poa_run: spoa's public flow (vendor/spoa/test/spoa_test.cpp:38-52) -- sequences in the order given, each
//     aligned against the WHOLE graph (sequence 0 against the empty graph: an empty alignment), AddAlignment with the quality
//     overload where a sequence has one (weights vc_weight_lut, graph.cpp:160-171) and weight 1 otherwise, GenerateConsensus at
//     the end (graph.cpp:450-459, the heaviest bundle with branch completion).  One engine for every alignment of the batch,
//     kSW / kNW / kOV with the caller's scores: linear gaps (vc_poa_run), or linear, affine or convex ones as spoa's
//     Create(type, m, n, g, e, q, c) chooses (vc_poa_run_gaps; LArgs::gaps = GM of k_lg_fwd / k_lg_back <GM>: 0, 1, 2 with 1, 3
//     and 5 int32 planes per matrix cell, one body each).  None of the window rules apply: no rank sort, spans, subgraph,
//     UpdateAlignment, "< 3 sequences", prune, trim, window type or FASTA-backbone quirk; seq_begin / seq_end / win_fasta are
//     never uploaded.  An empty sequence adds nothing (graph.cpp:187-190); a group of none, or of empty ones only, has the
//     empty consensus (graph.cpp:534-537).
//   kOV (semi-global, sisd_alignment_engine.cpp:227-247, 350-358, 380-382) differs from kNW in three places: column 0 of every
//   graph row is 0 (row 0 stays j * g); the end cell is the first maximum in (rank, column) order over the cells j >= 1 of the
//   sink rows; the backtrack stops at i == 0 || j == 0.
//
// Semantics: oracle/vc_oracle.c, function by function (the names below are the oracle's).  The order-sensitive parts -- the
// insertion order of in-/out-edges and aligned nodes, the DFS topological order, the DFS preorder of the largest component,
// the fp64 prune thresholds, average_weight (FASTA-backbone quirk included) and the tie rules of the backtrack and the heaviest
// bundle -- are restated literally.  Per-node lists are linked lists through the edges (in / out) and through cells (aligned
// nodes, edge labels) with head, tail and count per node, so appending keeps the oracle's order and nothing is ever moved.
//
// Kernels (gfx950, wave64), one launch per stage per alignment step over all windows in flight (lock-step, like vc_run's chunks):
//   k_lg_init   one lane per window: backbone chain, topological order, the backbone's share of average_weight (mode 2: the
//               empty graph, or at once the empty consensus of an empty group);
//   k_lg_prep   one lane per window: the next alignment of the window's schedule (subgraph of a partial-span layer when the
//               build needs one), its rank-ordered predecessor lists (CSR of row indices), row bytes and sink flags;
//   k_lg_fwd    <GM>, one wave per alignment: rows in rank order, columns over the 64 lanes; predecessor rows are read back from
//               the int32 planes (rows + 1) x (len + 1) in HBM; the horizontal move is a wave prefix maximum on tilted scores
//               (gap_scan), for every gap model;
//   k_lg_back   <GM>, one lane per alignment: walks the stored planes in the reference's order of candidates;
//   k_lg_apply  one lane per window: add-alignment + topological sort, or add-weights; prune + largest component at the end of
//               the build and of every round; the corrected sequence (mode 0), heaviest bundle + coverage + trim (mode 1) or the
//               heaviest bundle alone (mode 2).
//   k_lg_views  vc_poa_run_strand only, once per call, one lane per byte of the batch: the strand views (reverse complement, reversed
//               quality, the bytes complemented twice).  With them k_lg_fwd runs on a grid of (alignments, 2) -- one wave per
//               alignment and strand, the second strand's matrix behind the first's --, k_lg_back picks the strand by score and
//               walks the winner's matrix only, and k_lg_apply adds the kept view and records the choice (spoa's -s, main.cpp:287-304);
//   k_lg_msa    vc_poa_run_msa only, one wave per finished group: <0> node -> column by a wave prefix sum over the topological
//               order, <1> the rows ('-' fill, then a scatter over the edge labels), the consensus row and the coverage;
//   k_lg_graph  vc_poa_run_graph only, one wave per finished group: <0> the counts of the group's graph tables, <1> the tables --
//               nodes, out-edges as CSR, aligned pairs, a path per sequence, the consensus path (spoa's GFA and dot output).
//   The query stage, vc_poa_run_align only (spoa's engine->Align(sequence, graph, &score) for sequences that are NOT added), on the
//   finished groups while their tables are resident; every (group, query) pair is a job (LJob) and independent of the others:
//   k_lg_rows   one lane per finished group: the graph half of k_lg_prep (graph_rows) once per group, without a next sequence;
//   k_lg_qfwd   <GM>, a grid of (jobs of the launch, strands), one wave per job and strand: k_lg_fwd's rows (fwd_rows) on the query
//               batch's bytes or their reverse-complement view (k_lg_views on the query batch);
//   k_lg_qback  <GM>, one lane per job: k_lg_back's walk (back_walk) into the job's own pair area of rows + length pairs;
//   k_lg_qpack  one wave per job: the pairs compact behind the host's prefix offsets, nodes and positions apart.
//
// Limits, every schedule: a sequence is shorter than 65 535 bases; beyond that only the device memory bounds a window or group,
// and one whose tables or matrix it cannot hold at all comes back VC_WIN_OVERFLOW.  Where the reference throws (an invalid
// alignment, the score floor of WorstCaseAlignmentScore) that window or group is VC_WIN_INVALID and the rest are computed.
//
// Development knobs, read on every call of vc_large_run and vc_poa_run (unset: the behaviour above, and nothing is printed).  They only make tables and budgets
// smaller, so that the tests can reach the host schedule's rarer paths with small windows:
//   VC_LARGE_CAPS=n:4,a:6   a table starts at max(1, size >> shift): n nodes, e edges, a aligned cells, l labels, s stack, p pairs
//                           (the stack then also grows from (nodes + edges + aligned) >> shift, not from the unshifted sum);
//   VC_LARGE_ARENA_MB=x     arena budget (window tables per group; a window above twice the budget is refused) in MiB, fractions allowed;
//   VC_LARGE_MAT_MB=x       matrix budget (int32 matrices, every plane and both strands, per forward launch) in MiB;
//   VC_LARGE_GRAPH_WALK=1   vc_poa_run_graph walks every path node by node (Node::Successor) instead of scattering and compacting it;
//   VC_LARGE_LOG=1          one stderr line per event: "vc_large: regrow window=W flags=nodes,... caps n=.. e=.. a=.. l=.. s=.. p=..",
//                           "vc_large: group windows=N bytes=B ids=W,.. need=B,..", "vc_large: step launches=K over=O" (steps of more than one
//                           launch; O launches hold one matrix above the budget), "vc_large: refuse window=W bytes=B budget=B",
//                           "vc_large: msa launches=K bytes=B" (vc_poa_run_msa with flags: k_lg_msa<1> launches, bytes copied out),
//                           "vc_large: graph launches=K bytes=B" (vc_poa_run_graph: k_lg_graph<1> launches, bytes copied out),
//                           "vc_large: align jobs=J launches=K cells=C bytes=B" (vc_poa_run_align with queries: the queries of the
//                           groups that finished, k_lg_qfwd launches, their rows x columns with both strands counted, bytes copied out),
//                           and at the end of a call "vc_large: done alignments=A cells=C" (forward passes of the build, their rows x
//                           columns summed; a regrown window's are counted again; vc_poa_run_strand counts both strands' passes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "vechat_hip.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int32_t KNEG = INT32_MIN + 1024;             // the reference's engines' floor (oracle: KNEG)
constexpr int64_t TNEG = INT64_MIN / 4;                // tilted score of a lane beyond the sequence
constexpr uint32_t kCols = 8;                          // consecutive columns per lane in k_lg_fwd

enum : uint32_t { PH_BUILD = 0, PH_ROUND = 1, PH_FINAL = 2, PH_DONE = 3 };
// which table filled (LWin::grow): the host doubles it and runs the window again
enum : uint32_t { G_NODES = 1, G_EDGES = 2, G_ALIGNED = 4, G_LABELS = 8, G_STACK = 16, G_PAIRS = 32 };

struct LGraph {
    uint32_t n_nodes, n_edges, n_al, n_lb, n_rank, nseq;
    uint32_t labels;                                   // 1: edges keep sequence labels (the racon-linear overload's coverage and k_lg_msa read them)
    uint8_t* code;                                     // [NC]
    uint32_t *in_h, *in_t, *in_n, *out_h, *out_t, *out_n, *al_h, *al_t, *al_n, *rank;   // [NC]
    uint32_t *tail, *head, *nx_in, *nx_out, *lb_h, *lb_t;                               // [EC]
    int64_t* weight;                                   // [EC]
    uint8_t* alive;                                    // [EC]
    uint32_t *al_v, *al_nx;                            // [AC] aligned-node cells
    uint32_t *lb_v, *lb_nx;                            // [LC] label cells
};

struct LWin {
    uint32_t s0, nseq, L, fasta;                       // window: first sequence, sequences, backbone length, if_fasta
    uint32_t NC, EC, AC, LC, SC, PC;                   // capacities
    uint32_t phase, j, k, cur, sub, grow, status;      // schedule; cur = graph slot of G / P; sub = the alignment ran on a subgraph
    uint32_t num_codes;
    double total, avg;
    uint32_t rows, qlen, qs, type;                     // the current alignment: graph rows, query length, query (sequence index), 0 SW / 1 NW / 2 OV
    int32_t m, x, g, e, q, c;                          // scores; e, q, c: the affine / convex ones (mode 2), g elsewhere
    uint32_t max_i[2], max_j[2], npairs, cons_n;       // end cell per strand ([1]: vc_poa_run_strand's reverse complement)
    int32_t score[2];                                  // spoa's *score per strand: the end cell's value, 0 where spoa does not write it
    uint32_t rev;                                      // the strand the backtrack kept (1: the reverse complement), 0 without strands
    LGraph gr[2];
    int32_t *coder, *decoder;                          // [256]
    uint8_t *mark, *ign;                               // [NC]
    uint32_t *stack;                                   // [SC]
    uint32_t *node_rank, *map, *g2s, *fr_v, *fr_e, *comp, *best, *pred, *stamp;   // [NC] (stamp: [nseq + 1])
    uint8_t* fr_p;                                     // [NC]
    int64_t* scores;                                   // [NC]
    uint8_t *rchar, *sink;                             // [NC]
    uint32_t *poff, *prank;                            // [NC + 1], [EC]
    int32_t* pairs;                                    // [2 PC]
    uint8_t* cons;                                     // [NC]
    // vc_poa_run_msa only (nullptr otherwise): spoa's sequences_, one entry per sequence that was added (label = index)
    uint32_t *sq_begin, *sq_member;                    // [nseq] begin node; index of the group member
    uint32_t msa_rows, row_size;                       // k_lg_msa<0>: rows and columns of the group's alignment
    uint32_t gr_cols, gr_path;                         // k_lg_graph<0>: columns of the alignment, path entries (bases of the added sequences)
};

struct LArgs {
    LWin* win;
    uint32_t n;
    const uint64_t* seq_off;
    const uint32_t *seq_begin, *seq_end;
    const uint8_t *has_qual, *bases, *quals;
    const uint32_t* lut_w;                             // vc_weight_lut
    const double* lut_d;                               // 1 - 10^((33 - q) / 10), window.cpp:235,295
    int32_t match, mismatch, gap, sw_match, sw_mismatch, sw_gap;
    double min_conf, min_sup;
    uint32_t num_prune, mode, trim, window_type;       // mode 0 haplotype, 1 racon-linear, 2 POA group
    uint32_t algorithm;                                // mode 2: spoa::AlignmentType of every alignment (0 kSW, 1 kNW, 2 kOV)
    uint32_t gaps;                                     // mode 2: spoa::AlignmentSubtype (0 linear, 1 affine, 2 convex); 0 elsewhere
    int32_t gap_e, gap_q, gap_c;                       // mode 2: spoa's e, q, c after Create's subtype rule
    uint32_t msa;                                      // mode 2: VC_POA_MSA | VC_POA_MSA_CONSENSUS | VC_POA_COVERAGE, 0 elsewhere
    uint32_t graph;                                    // mode 2, vc_poa_run_graph: 1 paths by scatter and compaction, 2 by the literal walk; 0 elsewhere
    // mode 2, vc_poa_run_strand (strand = 1; nullptr / 0 elsewhere): the strand views of the batch, k_lg_views, laid out as bases /
    // quals are, and the choice per sequence of the batch
    uint32_t strand;
    uint8_t *rc_bases, *rv_quals, *rt_bases;           // reverse complement, reversed quality, the bytes complemented twice
    uint8_t* s_rev;                                    // [sequences] 1: the reverse complement was kept
    int32_t *s_score, *s_score_rev;                    // [sequences] both strands' scores
    uint64_t nbytes;                                   // k_lg_views: bytes of the batch
    // k_lg_fwd / k_lg_back: windows of this launch and their matrices (k_lg_msa<1>, k_lg_graph<1>: groups and the byte offsets of
    // their blocks in msa_out; k_lg_graph<1> has the offsets of the groups' scratch behind them, at hoff[groups + k])
    const uint32_t* list;
    const uint64_t* hoff;
    int32_t* H;
    uint8_t* msa_out;
    // vc_poa_run_align only (nullptr elsewhere): the jobs of the query stage (k_lg_qfwd / k_lg_qback: a.list holds job indices), the
    // query batch's offsets and bytes, its reverse-complement view (VC_POA_ALIGN_STRANDS), the jobs' pair areas and the packed pairs
    struct LJob* job;
    const uint64_t* q_off;
    const uint8_t *q_bases, *q_rc;
    int32_t *q_pairs, *q_out;
};

// One query against the finished graph of its group (vc_poa_run_align): filled by the host but for the results.
struct LJob {
    uint32_t win, qs;                                  // the group (index among the windows in flight), the query (sequence of the query batch)
    uint32_t rows, qlen, status;                       // graph rows, query length; VC_WIN_OK, or VC_WIN_INVALID from the backtrack
    uint32_t max_i[2], max_j[2];                       // end cell per strand
    int32_t score[2];                                  // spoa's *score per strand
    uint32_t rev, npairs;                              // the strand the backtrack walked, its pairs
    uint64_t area, pair_off;                           // pairs: first of the job's area (rows + qlen of them) in q_pairs, first in q_out
};

// ------------------------------------------------------------------ graph tables
__device__ uint32_t add_node(LWin& W, LGraph& g, uint32_t code) {
    if (g.n_nodes >= W.NC) { W.grow |= G_NODES; return NONE; }
    const uint32_t id = g.n_nodes++;
    g.code[id] = (uint8_t)code;
    g.in_h[id] = g.in_t[id] = g.out_h[id] = g.out_t[id] = g.al_h[id] = g.al_t[id] = NONE;
    g.in_n[id] = g.out_n[id] = g.al_n[id] = 0;
    return id;
}

__device__ bool push_label(LWin& W, LGraph& g, uint32_t e, uint32_t label) {
    if (!g.labels) return true;
    if (g.n_lb >= W.LC) { W.grow |= G_LABELS; return false; }
    const uint32_t c = g.n_lb++;
    g.lb_v[c] = label; g.lb_nx[c] = NONE;
    if (g.lb_t[e] == NONE) g.lb_h[e] = c; else g.lb_nx[g.lb_t[e]] = c;
    g.lb_t[e] = c;
    return true;
}

__device__ bool push_aligned(LWin& W, LGraph& g, uint32_t v, uint32_t a) {
    if (g.n_al >= W.AC) { W.grow |= G_ALIGNED; return false; }
    const uint32_t c = g.n_al++;
    g.al_v[c] = a; g.al_nx[c] = NONE;
    if (g.al_t[v] == NONE) g.al_h[v] = c; else g.al_nx[g.al_t[v]] = c;
    g.al_t[v] = c; g.al_n[v]++;
    return true;
}

// g_new_edge
__device__ bool new_edge(LWin& W, LGraph& g, uint32_t tail, uint32_t head, uint32_t label, uint32_t w) {
    if (g.n_edges >= W.EC) { W.grow |= G_EDGES; return false; }
    const uint32_t e = g.n_edges++;
    g.tail[e] = tail; g.head[e] = head; g.weight[e] = (int64_t)w; g.alive[e] = 1;
    g.nx_in[e] = g.nx_out[e] = NONE; g.lb_h[e] = g.lb_t[e] = NONE;
    if (!push_label(W, g, e, label)) return false;
    if (g.out_t[tail] == NONE) g.out_h[tail] = e; else g.nx_out[g.out_t[tail]] = e;
    g.out_t[tail] = e; g.out_n[tail]++;
    if (g.in_t[head] == NONE) g.in_h[head] = e; else g.nx_in[g.in_t[head]] = e;
    g.in_t[head] = e; g.in_n[head]++;
    return true;
}

// g_add_edge: find by head in tail's out-list, else append
__device__ bool add_edge(LWin& W, LGraph& g, uint32_t tail, uint32_t head, uint32_t w) {
    for (uint32_t e = g.out_h[tail]; e != NONE; e = g.nx_out[e]) {
        if (g.head[e] == head) {
            if (!push_label(W, g, e, g.nseq)) return false;
            g.weight[e] += (int64_t)w;
            return true;
        }
    }
    return new_edge(W, g, tail, head, g.nseq, w);
}

// The bytes a step reads of sequence s.  Without strands: the batch's.  vc_poa_run_strand: strand 1 aligns the reverse complement;
// what is added to the graph is the kept view -- the reverse complement with the reversed quality, or the forward strand
// complemented twice (main.cpp:297-299; its alignment was computed on the batch's own bytes).
__device__ __forceinline__ const uint8_t* aligned_bases(const LArgs& a, uint32_t s, uint32_t strand) {
    return (strand ? a.rc_bases : a.bases) + a.seq_off[s];
}
__device__ __forceinline__ const uint8_t* kept_bases(const LArgs& a, const LWin& W, uint32_t s) {
    return (a.strand ? (W.rev ? a.rc_bases : a.rt_bases) : a.bases) + a.seq_off[s];
}

__device__ __forceinline__ uint32_t weight_of(const LArgs& a, const LWin& W, uint32_t s, uint32_t i, bool use_qual) {
    return use_qual ? a.lut_w[(a.strand && W.rev ? a.rv_quals : a.quals)[a.seq_off[s] + i]] : 1u;
}

// g_add_chain: fresh chain for seq[begin, end); *first = first node or NONE
__device__ bool add_chain(const LArgs& a, LWin& W, LGraph& g, uint32_t s, bool uq, uint32_t begin, uint32_t end, uint32_t* first) {
    *first = NONE;
    const uint8_t* seq = kept_bases(a, W, s);
    uint32_t prev = NONE;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t curr = add_node(W, g, (uint32_t)W.coder[seq[i]]);
        if (curr == NONE) return false;
        if (*first == NONE) *first = curr;
        if (prev != NONE && !add_edge(W, g, prev, curr, weight_of(a, W, s, i - 1, uq) + weight_of(a, W, s, i, uq))) return false;
        prev = curr;
    }
    return true;
}

// g_toposort: iterative DFS over ids in order; in-edge tails then aligned nodes pushed; a node is emitted followed by its aligned nodes
__device__ bool toposort(LWin& W, LGraph& g) {
    g.n_rank = 0;
    const uint32_t N = g.n_nodes;
    uint8_t* marks = W.mark;
    uint8_t* ignored = W.ign;
    for (uint32_t v = 0; v < N; ++v) { marks[v] = 0; ignored[v] = 0; }
    uint32_t sp = 0;
    for (uint32_t s = 0; s < N; ++s) {
        if (marks[s] != 0) continue;
        if (sp >= W.SC) { W.grow |= G_STACK; return false; }
        W.stack[sp++] = s;
        while (sp) {
            const uint32_t c = W.stack[sp - 1];
            bool valid = true;
            if (marks[c] != 2) {
                for (uint32_t e = g.in_h[c]; e != NONE; e = g.nx_in[e]) {
                    const uint32_t t = g.tail[e];
                    if (marks[t] != 2) {
                        if (sp >= W.SC) { W.grow |= G_STACK; return false; }
                        W.stack[sp++] = t; valid = false;
                    }
                }
                if (!ignored[c]) {
                    for (uint32_t q = g.al_h[c]; q != NONE; q = g.al_nx[q]) {
                        const uint32_t al = g.al_v[q];
                        if (marks[al] != 2) {
                            if (sp >= W.SC) { W.grow |= G_STACK; return false; }
                            W.stack[sp++] = al; ignored[al] = 1; valid = false;
                        }
                    }
                }
                if (valid) {
                    marks[c] = 2;
                    if (!ignored[c]) {
                        if (g.n_rank + 1 + g.al_n[c] > W.NC) { W.grow |= G_NODES; return false; }   // (an aligned group is emitted once)
                        g.rank[g.n_rank++] = c;
                        for (uint32_t q = g.al_h[c]; q != NONE; q = g.al_nx[q]) g.rank[g.n_rank++] = g.al_v[q];
                    }
                } else {
                    marks[c] = 1;
                }
            }
            if (valid) sp--;
        }
    }
    return true;
}

// g_add_alignment.  Returns 0, -1 where the reference throws, -2 when a table filled.
__device__ int add_alignment(const LArgs& a, LWin& W, LGraph& g, const int32_t* A, uint32_t np, uint32_t s, bool uq) {
    const uint32_t len = (uint32_t)(a.seq_off[s + 1] - a.seq_off[s]);
    const uint8_t* seq = kept_bases(a, W, s);
    if (len == 0) return 0;
    for (uint32_t i = 0; i < len; ++i) {
        if (W.coder[seq[i]] == -1) {
            W.coder[seq[i]] = (int32_t)W.num_codes;
            W.decoder[W.num_codes++] = seq[i];
        }
    }
    uint32_t first;
    if (np == 0) {
        if (!add_chain(a, W, g, s, uq, 0, len, &first)) return -2;
        if (W.sq_begin) { W.sq_begin[g.nseq] = first; W.sq_member[g.nseq] = s - W.s0; }
        g.nseq++;
        return toposort(W, g) ? 0 : -2;
    }
    int32_t vfront = -1, vback = -1;
    for (uint32_t k = 0; k < np; ++k) {
        const int32_t q = A[2 * k + 1];
        if (q != -1) {
            if (q < 0 || q >= (int32_t)len) return -1;
            if (vfront == -1) vfront = q;
            vback = q;
        }
    }
    if (vfront == -1) return -1;
    uint32_t begin, last;
    if (!add_chain(a, W, g, s, uq, 0, (uint32_t)vfront, &begin)) return -2;
    uint32_t prev = (begin != NONE) ? g.n_nodes - 1 : NONE;
    if (!add_chain(a, W, g, s, uq, (uint32_t)vback + 1, len, &last)) return -2;
    for (uint32_t k = 0; k < np; ++k) {
        const int32_t n = A[2 * k], q = A[2 * k + 1];
        if (q == -1) continue;
        const uint32_t c = (uint32_t)W.coder[seq[q]];
        uint32_t curr = NONE;
        if (n == -1) {
            if ((curr = add_node(W, g, c)) == NONE) return -2;
        } else {
            const uint32_t jn = (uint32_t)n;
            if (jn >= g.n_nodes) return -1;
            if (g.code[jn] == c) {
                curr = jn;
            } else {
                for (uint32_t t = g.al_h[jn]; t != NONE; t = g.al_nx[t]) {
                    if (g.code[g.al_v[t]] == c) { curr = g.al_v[t]; break; }
                }
                if (curr == NONE) {
                    if ((curr = add_node(W, g, c)) == NONE) return -2;
                    // jn's own list only grows after the walk, so the walk sees the oracle's snapshot
                    for (uint32_t t = g.al_h[jn]; t != NONE; t = g.al_nx[t]) {
                        const uint32_t al = g.al_v[t];
                        if (!push_aligned(W, g, al, curr) || !push_aligned(W, g, curr, al)) return -2;
                    }
                    if (!push_aligned(W, g, jn, curr) || !push_aligned(W, g, curr, jn)) return -2;
                }
            }
        }
        if (begin == NONE) begin = curr;
        if (prev != NONE && !add_edge(W, g, prev, curr, weight_of(a, W, s, q - 1, uq) + weight_of(a, W, s, q, uq))) return -2;
        prev = curr;
    }
    if (last != NONE && !add_edge(W, g, prev, last, weight_of(a, W, s, vback, uq) + weight_of(a, W, s, vback + 1, uq))) return -2;
    if (W.sq_begin) { W.sq_begin[g.nseq] = begin; W.sq_member[g.nseq] = s - W.s0; }   // sequences_.emplace_back(begin), graph.cpp:296
    g.nseq++;
    return toposort(W, g) ? 0 : -2;
}

__device__ void reset_graph(LGraph& g) { g.n_nodes = g.n_edges = g.n_al = g.n_lb = g.n_rank = g.nseq = 0; }

// g_subgraph: the nodes reachable backwards from `end` (in-edges and aligned nodes) with id >= begin; W.map[new] = old
__device__ bool subgraph(LWin& W, const LGraph& g, LGraph& sub, uint32_t begin, uint32_t end) {
    const uint32_t N = g.n_nodes;
    uint8_t* in_sub = W.mark;
    for (uint32_t v = 0; v < N; ++v) in_sub[v] = 0;
    uint32_t sp = 0;
    W.stack[sp++] = end;
    while (sp) {
        const uint32_t c = W.stack[--sp];
        if (!in_sub[c] && c >= begin) {
            for (uint32_t e = g.in_h[c]; e != NONE; e = g.nx_in[e]) {
                if (sp >= W.SC) { W.grow |= G_STACK; return false; }
                W.stack[sp++] = g.tail[e];
            }
            for (uint32_t q = g.al_h[c]; q != NONE; q = g.al_nx[q]) {
                if (sp >= W.SC) { W.grow |= G_STACK; return false; }
                W.stack[sp++] = g.al_v[q];
            }
            in_sub[c] = 1;
        }
    }
    reset_graph(sub);
    sub.labels = 0;
    uint32_t nm = 0;
    for (uint32_t v = 0; v < N; ++v) {
        W.g2s[v] = NONE;
        if (!in_sub[v]) continue;
        if ((W.g2s[v] = add_node(W, sub, g.code[v])) == NONE) return false;
        W.map[nm++] = v;
    }
    for (uint32_t v = 0; v < N; ++v) {
        if (!in_sub[v]) continue;
        const uint32_t jt = W.g2s[v];
        for (uint32_t e = g.in_h[v]; e != NONE; e = g.nx_in[e]) {
            if (W.g2s[g.tail[e]] != NONE && !add_edge(W, sub, W.g2s[g.tail[e]], jt, (uint32_t)g.weight[e])) return false;
        }
        for (uint32_t q = g.al_h[v]; q != NONE; q = g.al_nx[q]) {
            if (W.g2s[g.al_v[q]] != NONE && !push_aligned(W, sub, jt, W.g2s[g.al_v[q]])) return false;
        }
    }
    return toposort(W, sub);
}

// g_prune (min_weight 0).  A decision reads weights only, never another edge's alive flag, so the tombstones are set in place.
__device__ void prune(LGraph& g, double d, double s, double avg) {
    for (uint32_t e = 0; e < g.n_edges; ++e) {
        if (!g.alive[e]) continue;
        if (g.weight[e] < 0) { g.alive[e] = 0; continue; }
        int64_t tot = 0;
        for (uint32_t o = g.out_h[g.tail[e]]; o != NONE; o = g.nx_out[o]) tot += g.weight[o];
        const double conf_uv = (double)g.weight[e] / (double)tot;
        const double support = (double)g.weight[e] / avg;
        tot = 0;
        for (uint32_t o = g.in_h[g.head[e]]; o != NONE; o = g.nx_in[o]) tot += g.weight[o];
        const double conf_vu = (double)g.weight[e] / (double)tot;
        if (!(conf_uv >= d && conf_vu >= d && support >= s)) g.alive[e] = 0;
    }
}

// g_dfs_component: recursive preorder with explicit frames; neighbours = live in-edge tails, then live out-edge heads
__device__ uint32_t dfs_component(LWin& W, const LGraph& g, uint32_t v0, uint32_t* comp) {
    uint8_t* visited = W.mark;
    uint32_t n = 0, sp = 0;
    visited[v0] = 1; comp[n++] = v0;
    W.fr_v[sp] = v0; W.fr_p[sp] = 0; W.fr_e[sp] = g.in_h[v0]; sp++;
    while (sp) {
        const uint32_t f = sp - 1;
        uint32_t u = NONE;
        while (u == NONE) {
            uint32_t e = W.fr_e[f];
            if (e == NONE) {
                if (W.fr_p[f] == 0) { W.fr_p[f] = 1; W.fr_e[f] = g.out_h[W.fr_v[f]]; continue; }
                break;
            }
            const bool in = W.fr_p[f] == 0;
            W.fr_e[f] = in ? g.nx_in[e] : g.nx_out[e];
            if (!g.alive[e]) continue;
            const uint32_t cand = in ? g.tail[e] : g.head[e];
            if (!visited[cand]) u = cand;
        }
        if (u == NONE) { sp--; continue; }
        visited[u] = 1; comp[n++] = u;
        W.fr_v[sp] = u; W.fr_p[sp] = 0; W.fr_e[sp] = g.in_h[u]; sp++;
    }
    return n;
}

// g_largest_subgraph: the last component of the largest size (`>=`), nodes in its DFS preorder, live out-edges without dedup
__device__ bool largest_subgraph(LWin& W, const LGraph& g, LGraph& sub) {
    const uint32_t N = g.n_nodes;
    for (uint32_t v = 0; v < N; ++v) W.mark[v] = 0;
    uint32_t *comp = W.comp, *best = W.best, best_size = 0;
    for (uint32_t v = 0; v < N; ++v) {
        if (W.mark[v]) continue;
        const uint32_t n = dfs_component(W, g, v, comp);
        if (n >= best_size) { best_size = n; uint32_t* t = best; best = comp; comp = t; }
    }
    reset_graph(sub);
    sub.labels = 0;
    for (uint32_t k = 0; k < best_size; ++k)
        if ((W.g2s[best[k]] = add_node(W, sub, g.code[best[k]])) == NONE) return false;
    for (uint32_t k = 0; k < best_size; ++k) {
        const uint32_t v = best[k];
        for (uint32_t e = g.out_h[v]; e != NONE; e = g.nx_out[e]) {
            if (!g.alive[e]) continue;
            if (!new_edge(W, sub, W.g2s[v], W.g2s[g.head[e]], 0, 0)) return false;
        }
    }
    return toposort(W, sub);
}

// g_add_weights
__device__ bool add_weights(const LArgs& a, LWin& W, LGraph& g, const int32_t* A, uint32_t np, uint32_t s, bool uq) {
    const uint32_t len = (uint32_t)(a.seq_off[s + 1] - a.seq_off[s]);
    if (len == 0 || np == 0) return true;
    uint32_t prev = NONE;
    for (uint32_t k = 0; k < np; ++k) {
        const int32_t n = A[2 * k], q = A[2 * k + 1];
        if (n == -1 || q == -1) { prev = NONE; continue; }
        const uint32_t curr = (uint32_t)n;
        if (prev != NONE && !add_edge(W, g, prev, curr, weight_of(a, W, s, q - 1, uq) + weight_of(a, W, s, q, uq))) return false;
        prev = curr;
    }
    return true;
}

// g_branch_completion
__device__ uint32_t branch_completion(LWin& W, const LGraph& g, uint32_t rank) {
    int64_t* scores = W.scores;
    uint32_t* pred = W.pred;
    const uint32_t start = g.rank[rank];
    for (uint32_t o = g.out_h[start]; o != NONE; o = g.nx_out[o]) {
        const uint32_t h = g.head[o];
        for (uint32_t e = g.in_h[h]; e != NONE; e = g.nx_in[e]) {
            if (g.tail[e] != start) scores[g.tail[e]] = -1;
        }
    }
    uint32_t mx = NONE;
    for (uint32_t i = rank + 1; i < g.n_rank; ++i) {
        const uint32_t it = g.rank[i];
        scores[it] = -1; pred[it] = NONE;
        for (uint32_t e = g.in_h[it]; e != NONE; e = g.nx_in[e]) {
            const uint32_t tl = g.tail[e];
            if (scores[tl] == -1) continue;
            if (scores[it] < g.weight[e] || (scores[it] == g.weight[e] && pred[it] != NONE && scores[pred[it]] <= scores[tl])) {
                scores[it] = g.weight[e]; pred[it] = tl;
            }
        }
        if (pred[it] != NONE) scores[it] += scores[pred[it]];
        if (mx == NONE || scores[mx] < scores[it]) mx = it;
    }
    return mx;
}

// g_heaviest_bundle -> W.comp[0 .. n) (node ids, source first)
__device__ uint32_t heaviest_bundle(LWin& W, const LGraph& g) {
    if (g.n_rank == 0) return 0;
    const uint32_t N = g.n_nodes;
    int64_t* scores = W.scores;
    uint32_t* pred = W.pred;
    for (uint32_t i = 0; i < N; ++i) { pred[i] = NONE; scores[i] = -1; }
    uint32_t mx = NONE;
    for (uint32_t r = 0; r < g.n_rank; ++r) {
        const uint32_t it = g.rank[r];
        for (uint32_t e = g.in_h[it]; e != NONE; e = g.nx_in[e]) {
            const uint32_t tl = g.tail[e];
            if (scores[it] < g.weight[e] || (scores[it] == g.weight[e] && pred[it] != NONE && scores[pred[it]] <= scores[tl])) {
                scores[it] = g.weight[e]; pred[it] = tl;
            }
        }
        if (pred[it] != NONE) scores[it] += scores[pred[it]];
        if (mx == NONE || scores[mx] < scores[it]) mx = it;
    }
    if (g.out_n[mx] != 0) {
        for (uint32_t r = 0; r < g.n_rank; ++r) W.node_rank[g.rank[r]] = r;
        while (g.out_n[mx] != 0) mx = branch_completion(W, g, W.node_rank[mx]);
    }
    uint32_t n = 0;
    while (pred[mx] != NONE) { W.comp[n++] = mx; mx = pred[mx]; }
    W.comp[n++] = mx;
    for (uint32_t x = 0, y = n - 1; x < y; ++x, --y) { const uint32_t t = W.comp[x]; W.comp[x] = W.comp[y]; W.comp[y] = t; }
    return n;
}

// g_coverage: distinct labels on v's in- and out-edges
__device__ uint32_t coverage(LWin& W, const LGraph& g, uint32_t v, uint32_t tick) {
    uint32_t cnt = 0;
    for (int dir = 0; dir < 2; ++dir) {
        for (uint32_t e = dir ? g.out_h[v] : g.in_h[v]; e != NONE; e = dir ? g.nx_out[e] : g.nx_in[e]) {
            for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) {
                const uint32_t l = g.lb_v[c];
                if (W.stamp[l] != tick) { W.stamp[l] = tick; cnt++; }
            }
        }
    }
    return cnt;
}

// the bases of the bundle's nodes W.comp[begin .. end] are the consensus, and the window or group is done
__device__ void write_consensus(LWin& W, const LGraph& G, int32_t begin, int32_t end) {
    W.cons_n = 0;
    for (int32_t i = begin; i <= end; ++i) W.cons[W.cons_n++] = (uint8_t)W.decoder[G.code[W.comp[i]]];
    W.status = VC_WIN_OK;
    W.phase = PH_DONE;
}

// window_linear after build_graph: heaviest bundle, coverage, TGS trim
__device__ void finish_linear(const LArgs& a, LWin& W) {
    const LGraph& G = W.gr[W.cur];
    const uint32_t n = heaviest_bundle(W, G);
    uint32_t* cov = W.best;
    for (uint32_t i = 0; i <= G.nseq; ++i) W.stamp[i] = 0;
    uint32_t tick = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = W.comp[i];
        cov[i] = coverage(W, G, v, ++tick);
        for (uint32_t q = G.al_h[v]; q != NONE; q = G.al_nx[q]) cov[i] += coverage(W, G, G.al_v[q], ++tick);
    }
    int32_t begin = 0, end = (int32_t)n - 1;
    if (a.window_type == 1 && a.trim) {
        const uint32_t avgc = (W.nseq - 1) / 2;
        for (; begin < (int32_t)n; ++begin) if (cov[begin] >= avgc) break;
        for (; end >= 0; --end) if (cov[end] >= avgc) break;
        if (begin >= end) { begin = 0; end = (int32_t)n - 1; }
    }
    write_consensus(W, G, begin, end);
}

// Graph::GenerateConsensus of a POA group (graph.cpp:450-459): the heaviest bundle, no coverage, no trim
__device__ void finish_poa(LWin& W) {
    const LGraph& G = W.gr[W.cur];
    write_consensus(W, G, 0, (int32_t)heaviest_bundle(W, G) - 1);
}

__device__ __forceinline__ bool full_span(const LArgs& a, const LWin& W, uint32_t s) {
    const uint32_t offset = (uint32_t)(0.01 * W.L);
    return a.seq_begin[s] < offset && a.seq_end[s] > W.L - offset;
}

__device__ void fail_window(LWin& W, uint32_t status) { W.status = status; W.phase = PH_DONE; W.rows = 0; }

// prune + largest component of G into the other slot (window_hap:715-719 / :738-743)
__device__ bool prune_and_keep_largest(const LArgs& a, LWin& W) {
    prune(W.gr[W.cur], a.min_conf, a.min_sup, W.avg);
    if (!largest_subgraph(W, W.gr[W.cur], W.gr[1 - W.cur])) return false;
    W.cur = 1 - W.cur;
    return true;
}

// AlignmentEngine::WorstCaseAlignmentScore (alignment_engine.cpp:101-110); e = q = c = g gives the linear engine's
__host__ __device__ inline int64_t worst_case(int64_t m, int64_t gp, int64_t ge, int64_t gq, int64_t gc, int64_t i, int64_t j) {
    auto gap_score = [&](int64_t len) -> int64_t {
        if (len == 0) return 0;
        const int64_t a = gp + (len - 1) * ge, b = gq + (len - 1) * gc;
        return a < b ? a : b;
    };
    const int64_t d = i > j ? i - j : j - i, mn = i < j ? i : j;
    const int64_t x = -1 * (m * mn + gap_score(d)), y = gap_score(i) + gap_score(j);
    return x < y ? x : y;
}

// ------------------------------------------------------------------ kernels
// biosoup::Sequence::ReverseAndComplement's byte rule (sequence.hpp:55-77): the complement is chosen on the upper-cased byte and is
// upper case; S, W, N and every byte without a complement stay as they are, in their own case.
__device__ __forceinline__ uint8_t complement(uint8_t c) {
    switch (c >= 'a' && c <= 'z' ? c - 32 : c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T': case 'U': return 'A';
        case 'R': return 'Y';
        case 'Y': return 'R';
        case 'K': return 'M';
        case 'M': return 'K';
        case 'B': return 'V';
        case 'D': return 'H';
        case 'H': return 'D';
        case 'V': return 'B';
        default: return c;
    }
}

// The strand views of vc_poa_run_strand, once per call, one lane per byte of the batch: byte x of sequence s (found by bisection
// of seq_off) goes, complemented, to the mirrored place of s in rc_bases, its quality to the same place of rv_quals, and,
// complemented twice, to its own place in rt_bases.
__global__ __launch_bounds__(256) void k_lg_views(LArgs a, uint32_t nseq) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= a.nbytes) return;
    uint32_t lo = 0, hi = nseq;                                            // the last s with seq_off[s] <= x
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.seq_off[mid] <= x) lo = mid; else hi = mid;
    }
    const uint64_t y = a.seq_off[lo] + (a.seq_off[lo + 1] - 1 - x);
    const uint8_t c = complement(a.bases[x]);
    a.rc_bases[y] = c;
    if (a.rv_quals) a.rv_quals[y] = a.quals[x];                            // (a query batch has neither: its bytes are only aligned)
    if (a.rt_bases) a.rt_bases[x] = complement(c);
}

__global__ __launch_bounds__(64) void k_lg_init(LArgs a) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    LWin& W = a.win[w];
    for (int c = 0; c < 256; ++c) { W.coder[c] = -1; W.decoder[c] = -1; }
    W.num_codes = 0;
    reset_graph(W.gr[0]); reset_graph(W.gr[1]);
    W.gr[0].labels = a.mode == 1 || a.msa != 0 || a.graph != 0; W.gr[1].labels = 0;
    W.cur = 0; W.sub = 0; W.grow = 0; W.status = 0xFF; W.rows = 0; W.npairs = 0; W.cons_n = 0; W.total = 0.0; W.avg = 0.0;
    W.msa_rows = 0; W.row_size = 0; W.rev = 0; W.gr_cols = 0; W.gr_path = 0;
    if (a.mode == 2) {                                                     // POA group: sequence 0 meets the empty graph in k_lg_prep
        W.phase = PH_BUILD; W.j = 0; W.k = 0;
        if (W.nseq == 0) finish_poa(W);                                    // no sequence: the empty consensus
        return;
    }
    if (W.nseq < 3) {                                                      // window.cpp:188-192: the backbone, unpolished
        if (W.L > W.NC) { W.grow |= G_NODES; return; }                    // cons holds NC bytes (only a shrunk table is shorter)
        const uint8_t* bb = a.bases + a.seq_off[W.s0];
        for (uint32_t i = 0; i < W.L; ++i) W.cons[i] = bb[i];
        W.cons_n = W.L;
        fail_window(W, VC_WIN_UNPOLISHED);
        return;
    }
    const int rc = add_alignment(a, W, W.gr[0], nullptr, 0, W.s0, true);  // the backbone always takes the quality overload
    if (rc == -2) return;
    if (rc) { fail_window(W, VC_WIN_INVALID); return; }
    if (a.mode == 0) {
        if (W.fasta) W.total += (double)W.L;
        else for (uint32_t q = 0; q < W.L; ++q) W.total += a.lut_d[a.quals[a.seq_off[W.s0] + q]];
    }
    W.phase = PH_BUILD; W.j = 1; W.k = 0;
}

// The graph half of an alignment's preparation, over graph g of W: node -> rank, and per rank the row byte, the sink flag and the
// predecessor rows (CSR of row indices, in in-edge order).  false: the topological order does not cover the graph.
__device__ bool graph_rows(LWin& W, const LGraph& g) {
    const uint32_t N = g.n_nodes;
    if (g.n_rank != N) return false;                                       // the rows below read rank[0 .. N)
    for (uint32_t r = 0; r < N; ++r) W.node_rank[g.rank[r]] = r;
    uint32_t cnt = 0;
    for (uint32_t r = 0; r < N; ++r) {
        const uint32_t v = g.rank[r];
        W.rchar[r] = (uint8_t)W.decoder[g.code[v]];
        W.sink[r] = g.out_n[v] == 0;
        W.poff[r] = cnt;
        for (uint32_t e = g.in_h[v]; e != NONE; e = g.nx_in[e]) W.prank[cnt++] = W.node_rank[g.tail[e]] + 1;
    }
    W.poff[N] = cnt;
    return true;
}

__global__ __launch_bounds__(64) void k_lg_prep(LArgs a) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    LWin& W = a.win[w];
    W.rows = 0; W.npairs = 0; W.max_i[0] = W.max_j[0] = W.max_i[1] = W.max_j[1] = 0; W.sub = 0;
    W.score[0] = W.score[1] = 0; W.rev = 0;                                // no forward pass: spoa leaves both scores at 0, forward is kept
    if (W.phase == PH_DONE || W.grow) return;
    uint32_t gi = W.cur;
    if (a.mode == 2) {                                                     // POA group: the next sequence against the whole graph
        W.qs = W.s0 + W.j;
        W.type = a.algorithm; W.m = a.match; W.x = a.mismatch; W.g = a.gap; W.e = a.gap_e; W.q = a.gap_q; W.c = a.gap_c;
    } else {
        bool nw = true;
        if (W.phase == PH_BUILD) {
            W.qs = W.s0 + W.j;
            if (!full_span(a, W, W.qs)) {
                if (!subgraph(W, W.gr[W.cur], W.gr[1 - W.cur], a.seq_begin[W.qs], a.seq_end[W.qs])) return;
                gi = 1 - W.cur; W.sub = 1;
            }
        } else if (W.phase == PH_ROUND) {
            W.qs = W.s0 + W.j;
            nw = W.j == 0 || full_span(a, W, W.qs);
        } else {
            W.qs = W.s0; nw = false;
        }
        W.type = nw ? 1 : 0;
        W.m = nw ? a.match : a.sw_match; W.x = nw ? a.mismatch : a.sw_mismatch; W.g = nw ? a.gap : a.sw_gap;
        W.e = W.q = W.c = W.g;
    }
    const LGraph& g = W.gr[gi];
    const uint32_t N = g.n_nodes, len = (uint32_t)(a.seq_off[W.qs + 1] - a.seq_off[W.qs]);
    if (N == 0 || len == 0) return;                                       // an empty alignment
    if (worst_case(W.m, W.g, W.e, W.q, W.c, (int64_t)len + 8, N) < (int64_t)KNEG) { fail_window(W, VC_WIN_INVALID); return; }
    if (!graph_rows(W, g)) { fail_window(W, VC_WIN_INVALID); return; }
    W.rows = N; W.qlen = len;
}

// The query stage's rows, once per finished group (vc_poa_run_align): the graph half of k_lg_prep without a next sequence.
__global__ __launch_bounds__(64) void k_lg_rows(LArgs a) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    LWin& W = a.win[w];
    if (W.phase != PH_DONE || W.grow || W.status != VC_WIN_OK) return;
    (void)graph_rows(W, W.gr[W.cur]);                                      // (the host has n_rank and n_nodes: it makes no job where they differ)
}

__device__ __forceinline__ bool better(int32_t s, uint32_t i, uint32_t j, int32_t bs, uint32_t bi, uint32_t bj) {
    return s > bs || (s == bs && (i < bi || (i == bi && j < bj)));
}

// The horizontal gap of a row as a wave scan: out[q] = max over the columns k < j of v[k] - k d, where column j = j0 + q, v holds
// this lane's kCols columns and carry the maximum over the chunks before (it starts at column 0's term and is updated here).
// Columns beyond the sequence need no test: they lie behind every real column, only in the last chunk, and a prefix maximum
// carries nothing backwards, so whatever v holds there reaches no real column (and the carry is not read again).
// Every lane calls it: it shuffles.
__device__ __forceinline__ void gap_scan(const int32_t (&v)[kCols], uint32_t j0, int32_t d, int64_t& carry, int64_t (&out)[kCols]) {
    const uint32_t lane = threadIdx.x;
    int64_t run = TNEG;
#pragma unroll
    for (uint32_t q = 0; q < kCols; ++q) {
        out[q] = run;
        const int64_t t = (int64_t)v[q] - (int64_t)(j0 + q) * d;
        if (t > run) run = t;
    }
    int64_t T = run;                                                   // inclusive scan of the lanes' maxima
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const int64_t o = __shfl_up(T, s, 64);                         // (a lane below s gets its own T back)
        if (o > T) T = o;
    }
    int64_t before = __shfl_up(T, 1, 64);                              // what the lanes in front (and the chunks before) reached
    if (lane == 0 || carry > before) before = carry;
    const int64_t last = __shfl(T, 63, 64);
    if (last > carry) carry = last;
#pragma unroll
    for (uint32_t q = 0; q < kCols; ++q) if (before > out[q]) out[q] = before;
}

// int32 planes per matrix cell under gap model gm (LArgs::gaps, the kernels' GM): H (, F, E (, O, Q))
__host__ __device__ constexpr uint32_t plane_count(uint32_t gm) { return gm == 0 ? 1 : gm == 1 ? 3 : 5; }

// The matrix of the alignment in slot `slot` of a launch, strand st: plane_count(GM) planes of (rows + 1) x (len + 1) int32 each,
// one behind the other, strand 1's behind strand 0's.  w: cells per row.  A plane GM does not have is nullptr.
struct Mat { uint64_t w; int32_t *H, *F, *E, *O, *Q; };

template <uint32_t GM>
__device__ __forceinline__ Mat matrix_of(const LArgs& a, uint32_t slot, uint32_t rows, uint32_t len, uint32_t st) {
    Mat M{};
    M.w = (uint64_t)len + 1;
    const uint64_t P = ((uint64_t)rows + 1) * M.w;
    M.H = a.H + a.hoff[slot] + st * plane_count(GM) * P;
    if constexpr (GM >= 1) { M.F = M.H + P; M.E = M.F + P; }
    if constexpr (GM == 2) { M.O = M.E + P; M.Q = M.O + P; }
    return M;
}

// What a forward pass and a backtrack read of their alignment, whoever asks for it -- a step of the build (view_of, from the
// window) or a query of vc_poa_run_align (query_view, from the job): the size, the engine, the sequence's bytes, the row tables
// of graph_rows and rank -> node id.
struct AlnView {
    uint32_t rows, len, type;                          // graph rows, sequence length, 0 SW / 1 NW / 2 OV
    int32_t m, x, g, e, q, c;
    const uint8_t* seq;
    const uint32_t *poff, *prank;
    const uint8_t *rchar, *sink;
    const uint32_t* rank;
};
struct EndCell { int32_t s; uint32_t i, j; };

__device__ __forceinline__ AlnView view_of(const LArgs& a, const LWin& W, uint32_t st) {
    return AlnView{W.rows, W.qlen, W.type, W.m, W.x, W.g, W.e, W.q, W.c, aligned_bases(a, W.qs, st),
                   W.poff, W.prank, W.rchar, W.sink, W.gr[W.sub ? 1 - W.cur : W.cur].rank};
}
__device__ __forceinline__ AlnView query_view(const LArgs& a, const LWin& W, const LJob& J, uint32_t st) {
    return AlnView{J.rows, J.qlen, a.algorithm, a.match, a.mismatch, a.gap, a.gap_e, a.gap_q, a.gap_c,
                   (st ? a.q_rc : a.q_bases) + a.q_off[J.qs], W.poff, W.prank, W.rchar, W.sink, W.gr[W.cur].rank};
}

// g_align's forward pass with linear (GM 0, sisd_alignment_engine.cpp:292-367), affine (GM 1, :462-540) or convex (GM 2,
// :678-770) gaps and Initialize (:120-246): one wave per alignment and strand.  Row i = rank i - 1; lane l holds columns
// 512 c + 8 l + 1 .. + 8 of chunk c.  The planes hold spoa's values cell for cell, the kNegativeInfinity borders and column 0's
// F / O chains included: the backtrack compares them for equality.  A row is stored and the next may read it after the barrier.
// Per row: x[j] = max(diagonal, F[j] (, O[j]) (, 0 for kSW)) over every predecessor row -- SW clamps first, C[j] = max(0, x[j],
// C[j-1] + g) being the plain recurrence on max(0, x) --; then the horizontal gaps.  Since g <= e, E[j] = max(max_k<j (H[k] + g +
// (j - 1 - k) e), kNegativeInfinity + j e) equals the same maximum over x[k] with x[0] = H[i][0]: one exclusive prefix maximum of
// the tilted x[k] - k e (gap_scan, carried from chunk to chunk) gives E and H = max(x, E).
// GM 0 is that recurrence with e = g and H alone: the vertical term is H + g, column 0's chain lives in H itself, nothing but H
// is stored, and column 0's scan term max(H[i][0], kNegativeInfinity - g + e) is H[i][0] (k_lg_prep's worst-case check keeps
// every score above kNegativeInfinity).
// Convex: H comes out of the two scans over x, (g, e) and (q, c), but E and Q do not (E may extend a gap opened in Q and vice
// versa), so they are scanned a second time over the final H.
// kOV: column 0 of a graph row is 0 instead of the vertical chain (so the horizontal move starts from 0), and every cell of a
// sink row is an end-cell candidate, not only the last column.
// The body is fwd_rows, shared by k_lg_fwd (a step of the build) and k_lg_qfwd (a query against a finished graph): every lane
// of the wave calls it and every lane gets the end cell back.
template <uint32_t GM>
__device__ __forceinline__ EndCell fwd_rows(const AlnView& W, const Mat& M) {
    const uint32_t lane = threadIdx.x;
    const uint32_t N = W.rows, len = W.len;
    const uint64_t w = M.w;
    int32_t *const H = M.H, *const F = M.F, *const E = M.E, *const O = M.O, *const Q = M.Q;
    const bool sw = W.type == 0, ov = W.type == 2;
    const int32_t m = W.m, x = W.x, gp = W.g, ge = GM == 0 ? gp : W.e, gq = W.q, gc = W.c;
    const uint8_t* seq = W.seq;
    auto vertical = [&](uint64_t c) -> int32_t {                       // F's term from cell c of a predecessor row
        if constexpr (GM == 0) return H[c] + gp;
        else return max(H[c] + gp, F[c] + ge);
    };
    for (uint32_t j = lane; j <= len; j += 64) {                       // row 0
        const int32_t ej = j == 0 ? 0 : gp + (int32_t)(j - 1) * ge;
        int32_t h = ej;
        if constexpr (GM >= 1) { F[j] = j == 0 ? 0 : KNEG; E[j] = ej; }
        if constexpr (GM == 2) {
            const int32_t qj = j == 0 ? 0 : gq + (int32_t)(j - 1) * gc;
            O[j] = j == 0 ? 0 : KNEG;
            Q[j] = qj;
            h = max(ej, qj);
        }
        H[j] = (sw || j == 0) ? 0 : h;
    }
    __syncthreads();
    int32_t bs = sw ? 0 : KNEG;
    uint32_t bi = 0, bj = 0;
    for (uint32_t r = 0; r < N; ++r) {
        const uint64_t i = (uint64_t)r + 1, ro = i * w;
        const uint32_t po = W.poff[r], pe = W.poff[r + 1];
        const uint8_t ch = W.rchar[r];
        const bool sink = W.sink[r] != 0;
        const int32_t* F0 = GM == 0 ? H : F;                           // column 0's vertical chain
        int32_t f0 = pe == po ? gp - ge : KNEG, o0 = pe == po ? gq - gc : KNEG;
        for (uint32_t k = po; k < pe; ++k) {
            f0 = max(f0, F0[(uint64_t)W.prank[k] * w]);
            if constexpr (GM == 2) o0 = max(o0, O[(uint64_t)W.prank[k] * w]);
        }
        f0 += ge; o0 += gc;
        const int32_t h0 = (sw || ov) ? 0 : (GM == 2 ? max(o0, f0) : f0);
        if (lane == 0) {
            H[ro] = h0;
            if constexpr (GM >= 1) { F[ro] = f0; E[ro] = KNEG; }
            if constexpr (GM == 2) { O[ro] = o0; Q[ro] = KNEG; }
        }
        // column 0's terms of the scans, kNegativeInfinity's chain (E[i][0] + j e) beside H[i][0]
        int64_t cxe = max((int64_t)h0, (int64_t)KNEG - gp + ge), cxq = max((int64_t)h0, (int64_t)KNEG - gq + gc);
        int64_t che = cxe, chq = cxq;
        // a chunk is 64 lanes x kCols consecutive columns: the prefix maximum runs inside a lane first, then once across the lanes
        for (uint32_t cb = 0; cb < len; cb += 64 * kCols) {
            const uint32_t j0 = cb + lane * kCols + 1;
            int32_t xv[kCols];
#pragma unroll
            for (uint32_t q = 0; q < kCols; ++q) {
                const uint32_t j = j0 + q;
                xv[q] = KNEG;
                if (j > len) continue;
                const int32_t s = seq[j - 1] == ch ? m : x;
                uint64_t p = pe == po ? 0 : (uint64_t)W.prank[po] * w;
                int32_t d = H[p + j - 1] + s, f = vertical(p + j), o = KNEG;
                if constexpr (GM == 2) o = max(H[p + j] + gq, O[p + j] + gc);
                for (uint32_t k = po + 1; k < pe; ++k) {
                    p = (uint64_t)W.prank[k] * w;
                    d = max(d, H[p + j - 1] + s);
                    f = max(f, vertical(p + j));
                    if constexpr (GM == 2) o = max(o, max(H[p + j] + gq, O[p + j] + gc));
                }
                int32_t v = max(d, f);
                if constexpr (GM >= 1) F[ro + j] = f;
                if constexpr (GM == 2) { O[ro + j] = o; v = max(v, o); }
                if (sw) v = max(v, 0);
                xv[q] = v;
            }
            int64_t se[kCols], sq[kCols];
            int32_t hv[kCols];
            gap_scan(xv, j0, ge, cxe, se);
            if constexpr (GM == 2) gap_scan(xv, j0, gc, cxq, sq);
#pragma unroll
            for (uint32_t q = 0; q < kCols; ++q) {
                const int64_t j = (int64_t)(j0 + q);
                int64_t h = max((int64_t)xv[q], se[q] + (gp - ge) + j * ge);
                if constexpr (GM == 2) h = max(h, sq[q] + (gq - gc) + j * gc);
                hv[q] = (int32_t)h;
            }
            if constexpr (GM == 2) {                                   // E and Q over the final H
                gap_scan(hv, j0, ge, che, se);
                gap_scan(hv, j0, gc, chq, sq);
            }
#pragma unroll
            for (uint32_t q = 0; q < kCols; ++q) {
                const uint32_t j = j0 + q;
                if (j > len) break;
                const int32_t h = hv[q];
                H[ro + j] = h;
                if constexpr (GM >= 1) E[ro + j] = (int32_t)(se[q] + (gp - ge) + (int64_t)j * ge);
                if constexpr (GM == 2) Q[ro + j] = (int32_t)(sq[q] + (gq - gc) + (int64_t)j * gc);
                if (sw ? h > bs : (sink && (ov || j == len) && h > bs)) { bs = h; bi = (uint32_t)i; bj = j; }
            }
        }
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int32_t os = __shfl_xor(bs, d, 64);
        const uint32_t oi = __shfl_xor(bi, d, 64), oj = __shfl_xor(bj, d, 64);
        if (better(os, oi, oj, bs, bi, bj)) { bs = os; bi = oi; bj = oj; }
    }
    return EndCell{bs, bi, bj};
}

template <uint32_t GM>
__global__ __launch_bounds__(64) void k_lg_fwd(LArgs a) {
    LWin& W = a.win[a.list[blockIdx.x]];
    const uint32_t st = blockIdx.y;                                    // the strand
    const EndCell b = fwd_rows<GM>(view_of(a, W, st), matrix_of<GM>(a, blockIdx.x, W.rows, W.qlen, st));
    if (threadIdx.x == 0) { W.max_i[st] = b.i; W.max_j[st] = b.j; W.score[st] = b.s; }
}

// A query of vc_poa_run_align against the finished graph of its group: the same rows on a grid of (jobs of the launch, strands),
// the bytes from the query batch or its reverse-complement view, the result in the job.
template <uint32_t GM>
__global__ __launch_bounds__(64) void k_lg_qfwd(LArgs a) {
    LJob& J = a.job[a.list[blockIdx.x]];
    const uint32_t st = blockIdx.y;
    const EndCell b = fwd_rows<GM>(query_view(a, a.win[J.win], J, st), matrix_of<GM>(a, blockIdx.x, J.rows, J.qlen, st));
    if (threadIdx.x == 0) { J.max_i[st] = b.i; J.max_j[st] = b.j; J.score[st] = b.s; }
}

// g_align's backtrack, one lane per alignment, in the reference's order of candidates, literally.
// GM 0 (Linear, sisd_alignment_engine.cpp:369-460): the diagonal from each predecessor (in in-edge order), vertical likewise, then
// horizontal; one pair per step.
// GM 1 (Affine, :542-676) and GM 2 (Convex, :780-925): the diagonal over the in-edges; then vertical (extend_up when H == F + e /
// O + c of a predecessor, an opening when H == H + g / + q); then horizontal (extend_left from E / Q likewise); then the inner
// loops that emit a whole gap run.  Affine's vertical run stops on F == H + g; convex's tries the extensions over every in-edge
// first, then the openings (prev_i = 0 when none is found).
// The body is back_walk, shared by k_lg_back and k_lg_qback: from end cell (i, j), np pairs (node, position) into pairs[0 .. 2 cap)
// in sequence order.  Returns 0, 1 when the pairs do not fit, 2 where no candidate matches (cannot happen on a DAG).
template <uint32_t GM>
__device__ __forceinline__ int back_walk(const AlnView& W, const Mat& M, uint32_t i, uint32_t j, int32_t* pairs, uint32_t cap, uint32_t& np) {
    const uint64_t w = M.w;
    const int32_t *const H = M.H, *const F = M.F, *const E = M.E, *const O = M.O, *const Q = M.Q;
    const uint32_t* rank = W.rank;
    const uint8_t* seq = W.seq;
    const bool sw = W.type == 0, ov = W.type == 2;
    const int32_t gp = W.g, ge = W.e, gq = W.q, gc = W.c;
    np = 0;
    auto emit = [&](int32_t node, int32_t pos) -> bool {
        if (np >= cap) return false;
        pairs[2 * np] = node; pairs[2 * np + 1] = pos;
        ++np;
        return true;
    };
    for (;;) {
        if (sw) { if (H[(uint64_t)i * w + j] == 0) break; }
        else if (ov) { if (i == 0 || j == 0) break; }
        else if (i == 0 && j == 0) break;
        const int32_t Hij = H[(uint64_t)i * w + j];
        uint32_t pi = 0, pj = 0;
        bool found = false, up = false, left = false;
        const uint32_t po = i ? W.poff[i - 1] : 0, pe = i ? W.poff[i] : 0;
        const uint32_t ncand = pe > po ? pe - po : 1;                      // a row without predecessors follows row 0
        if (i != 0 && j != 0) {
            const int32_t s = seq[j - 1] == W.rchar[i - 1] ? W.m : W.x;
            for (uint32_t k = 0; k < ncand; ++k) {
                const uint32_t p = pe > po ? W.prank[po + k] : 0;
                if (Hij == H[(uint64_t)p * w + (j - 1)] + s) { pi = p; pj = j - 1; found = true; break; }
            }
        }
        if (!found && i != 0) {
            for (uint32_t k = 0; k < ncand; ++k) {
                const uint64_t c = (uint64_t)(pe > po ? W.prank[po + k] : 0) * w + j;
                if constexpr (GM == 0) found = Hij == H[c] + gp;
                else if constexpr (GM == 1) found = (up = Hij == F[c] + ge) || Hij == H[c] + gp;
                else found = (up = Hij == F[c] + ge) || Hij == H[c] + gp || (up = Hij == O[c] + gc) || Hij == H[c] + gq;
                if (found) { pi = (uint32_t)(c / w); pj = j; break; }
            }
        }
        if (!found && j != 0) {
            const uint64_t c = (uint64_t)i * w + j - 1;
            if constexpr (GM == 0) found = Hij == H[c] + gp;
            else if constexpr (GM == 1) found = (left = Hij == E[c] + ge) || Hij == H[c] + gp;
            else found = (left = Hij == E[c] + ge) || Hij == H[c] + gp || (left = Hij == Q[c] + gc) || Hij == H[c] + gq;
            if (found) { pi = i; pj = j - 1; }
        }
        if (!found) return 2;                                              // cannot happen on a DAG
        if (!emit(i == pi ? -1 : (int32_t)rank[i - 1], j == pj ? -1 : (int32_t)j - 1)) return 1;
        i = pi; j = pj;
        if constexpr (GM != 0) {
            if (left) {
                for (;;) {
                    if (j == 0) return 2;                                  // E[i][0] is kNegativeInfinity: cannot happen
                    if (!emit(-1, (int32_t)j - 1)) return 1;
                    --j;
                    const uint64_t c = (uint64_t)i * w + j;
                    if constexpr (GM == 1) { if (E[c] + ge != E[c + 1]) break; }
                    else { if (E[c] + ge != E[c + 1] && Q[c] + gc != Q[c + 1]) break; }
                }
            } else if (up) {
                for (;;) {
                    if (i == 0) return 2;                                  // F[0][j] is kNegativeInfinity: cannot happen
                    const uint64_t c = (uint64_t)i * w + j;
                    const uint32_t qo = W.poff[i - 1], qe = W.poff[i];
                    bool stop;
                    uint32_t prev = 0;
                    if constexpr (GM == 1) {
                        stop = false;
                        for (uint32_t k = qo; k < qe; ++k) {
                            const uint64_t pc = (uint64_t)W.prank[k] * w + j;
                            if ((stop = F[c] == H[pc] + gp) || F[c] == F[pc] + ge) { prev = W.prank[k]; break; }
                        }
                    } else {
                        stop = true;
                        for (uint32_t k = qo; k < qe; ++k) {
                            const uint64_t pc = (uint64_t)W.prank[k] * w + j;
                            if (F[c] == F[pc] + ge || O[c] == O[pc] + gc) { prev = W.prank[k]; stop = false; break; }
                        }
                        if (stop) {
                            for (uint32_t k = qo; k < qe; ++k) {
                                const uint64_t pc = (uint64_t)W.prank[k] * w + j;
                                if (F[c] == H[pc] + gp || O[c] == H[pc] + gq) { prev = W.prank[k]; break; }
                            }
                        }
                    }
                    if (!emit((int32_t)rank[i - 1], -1)) return 1;
                    i = prev;
                    if (stop || i == 0) break;
                }
            }
        }
    }
    for (uint32_t x = 0; x < np / 2; ++x) {
        const uint32_t y = np - 1 - x;
        const int32_t t0 = pairs[2 * x], t1 = pairs[2 * x + 1];
        pairs[2 * x] = pairs[2 * y]; pairs[2 * x + 1] = pairs[2 * y + 1];
        pairs[2 * y] = t0; pairs[2 * y + 1] = t1;
    }
    return 0;
}

template <uint32_t GM>
__global__ __launch_bounds__(64) void k_lg_back(LArgs a, uint32_t n) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    LWin& W = a.win[a.list[b]];
    // the strand: spoa keeps the forward one unless the reverse complement scores higher (main.cpp:297), and walks that matrix
    const uint32_t st = a.strand && W.score[0] < W.score[1];
    W.rev = st;
    W.npairs = 0;
    if (W.max_i[st] == 0 && W.max_j[st] == 0) return;                      // an empty alignment
    uint32_t np;
    const int rc = back_walk<GM>(view_of(a, W, st), matrix_of<GM>(a, b, W.rows, W.qlen, st), W.max_i[st], W.max_j[st], W.pairs, W.PC, np);
    if (rc == 1) { W.grow |= G_PAIRS; return; }
    if (rc == 2) { fail_window(W, VC_WIN_INVALID); return; }
    W.npairs = np;
}

// The backtrack of a query, one lane per job of the launch, into the job's own pair area: a step lowers the row, the column or
// both, so rows + length pairs always fit.  The strand rule is the build's (ties: as given).
template <uint32_t GM>
__global__ __launch_bounds__(64) void k_lg_qback(LArgs a, uint32_t n) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    LJob& J = a.job[a.list[b]];
    const uint32_t st = a.q_rc != nullptr && J.score[0] < J.score[1];
    J.rev = st;
    J.npairs = 0;
    if (J.max_i[st] == 0 && J.max_j[st] == 0) return;                      // an empty alignment
    uint32_t np;
    const int rc = back_walk<GM>(query_view(a, a.win[J.win], J, st), matrix_of<GM>(a, b, J.rows, J.qlen, st), J.max_i[st], J.max_j[st],
                                 a.q_pairs + 2 * J.area, J.rows + J.qlen, np);
    if (rc) { J.status = VC_WIN_INVALID; return; }
    J.npairs = np;
}

// The pairs of every job, compact: one wave per job reads its area (node, position interleaved) eight bytes per lane and writes
// a.q_out[pair_off ..) (nodes) and a.q_out[total + pair_off ..) (positions), consecutive lanes to consecutive words.
__global__ __launch_bounds__(64) void k_lg_qpack(LArgs a, uint64_t total) {
    const LJob& J = a.job[blockIdx.x];
    const int2* src = (const int2*)(a.q_pairs + 2 * J.area);
    int32_t *node = a.q_out + J.pair_off, *pos = a.q_out + total + J.pair_off;
    for (uint32_t k = threadIdx.x; k < J.npairs; k += 64) {
        const int2 p = src[k];
        node[k] = p.x; pos[k] = p.y;
    }
}

__global__ __launch_bounds__(64) void k_lg_apply(LArgs a) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    LWin& W = a.win[w];
    if (W.phase == PH_DONE || W.grow) return;
    const uint32_t s = W.qs, np = W.npairs;
    const bool hq = a.has_qual[s] != 0;
    if (W.phase == PH_BUILD) {
        if (W.sub)                                                         // UpdateAlignment, graph.cpp:734-745
            for (uint32_t k = 0; k < np; ++k) if (W.pairs[2 * k] != -1) W.pairs[2 * k] = (int32_t)W.map[W.pairs[2 * k]];
        const int rc = add_alignment(a, W, W.gr[W.cur], W.pairs, np, s, hq);
        if (rc == -2) return;
        if (rc) { fail_window(W, VC_WIN_INVALID); return; }
        if (a.strand) { a.s_rev[s] = (uint8_t)W.rev; a.s_score[s] = W.score[0]; a.s_score_rev[s] = W.score[1]; }
        if (a.mode == 0) {
            const uint32_t len = (uint32_t)(a.seq_off[s + 1] - a.seq_off[s]);
            if (!hq) W.total += (double)len;
            else for (uint32_t q = 0; q < len; ++q) W.total += a.lut_d[a.quals[a.seq_off[s] + q]];
        }
        if (++W.j < W.nseq) return;
        if (a.mode == 1) { finish_linear(a, W); return; }
        if (a.mode == 2) { finish_poa(W); return; }
        const uint16_t window_len = (uint16_t)W.L;                         // window.cpp:216
        W.avg = W.fasta ? 2.0 * W.total / window_len : 2.0 * W.total / window_len * 1000;
        if (!prune_and_keep_largest(a, W)) return;
        W.j = 0; W.k = 0;
        W.phase = a.num_prune > 1 ? PH_ROUND : PH_FINAL;
    } else if (W.phase == PH_ROUND) {
        // the backbone's qualities_[0].first is never nullptr: quality overload (a dummy '!' gives 0)
        if (!add_weights(a, W, W.gr[W.cur], W.pairs, np, s, W.j == 0 ? true : hq)) return;
        if (++W.j < W.nseq) return;
        if (!prune_and_keep_largest(a, W)) return;
        W.j = 0;
        if (++W.k + 1 >= a.num_prune) W.phase = PH_FINAL;
    } else {                                                               // GenerateCorrectedSequence, graph.cpp:1167-1179
        const LGraph& P = W.gr[W.cur];
        W.cons_n = 0;
        for (uint32_t k = 0; k < np; ++k) {
            if (W.pairs[2 * k] == -1) continue;
            W.cons[W.cons_n++] = (uint8_t)W.decoder[P.code[W.pairs[2 * k]]];
        }
        W.status = VC_WIN_OK;
        W.phase = PH_DONE;
    }
}

// Graph::GenerateMultipleSequenceAlignment (graph.cpp:393-448) and the summary of GenerateConsensus(&summary, false)
// (graph.cpp:476-484) of a finished POA group: one wave per group, no lane-serial stage.
//   PH 0, every group in flight: node -> column (InitializeMultipleSequenceAlignment) into W.map, W.row_size, W.msa_rows.  The
//     topological sort emits an aligned group as one block, the leader followed by its aligned list, and the reference gives a
//     block one column.  Aligned nodes are mutually aligned (add_alignment joins a new node to the whole group), so position i
//     opens a block exactly when rank[i - 1] is not an aligned node of rank[i]: a flag per position, a wave prefix sum over
//     tiles of 64 positions with a carried total, column = prefix - 1.
//   PH 1, the groups of a.list, block at a.msa_out + a.hoff[blockIdx.x]: msa_rows x row_size bytes, then (16-byte aligned)
//     msa_rows uint32, the group member of every row, then (16-byte aligned, VC_POA_COVERAGE) cons_n uint32.  The rows are filled with '-' by 16-byte stores, then the bases are scattered: the
//     reference walks Successor(i) from sequences_[i], which visits the begin node and the head of every edge that carries label
//     i -- a sequence's path has, at each of its nodes, exactly one out-edge with its label, and meets a node once -- so
//     row[label][column[head]] = decoder[code[head]] over all label cells writes the same bytes without the dependent chain.
//     Coverage: Node::Coverage() counts the distinct labels of a node's in- and out-edges.  A sequence enters and leaves a
//     node once, so no label repeats among the in-edges nor among the out-edges, and a label on an out-edge is missing from the
//     in-edges exactly when the sequence begins at the node: the count is the in-edge label cells plus the out-edge cells
//     whose sequence begins here.  Lanes take consensus positions.
// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(x, d, 64);
        if (lane >= d) x += o;
    }
    return x;
}

// PH 0 of k_lg_msa and of k_lg_graph: node -> column into W.map; returns the number of columns.  Every lane calls it.
__device__ uint32_t msa_columns(LWin& W, const LGraph& g, uint32_t lane) {
    const uint32_t N = g.n_rank;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < N; base += 64) {
        const uint32_t i = base + lane;
        uint32_t v = NONE, x = 0;
        if (i < N) {
            v = g.rank[i];
            x = 1;
            if (i > 0) {
                const uint32_t p = g.rank[i - 1];
                for (uint32_t q = g.al_h[v]; q != NONE; q = g.al_nx[q]) if (g.al_v[q] == p) { x = 0; break; }
            }
        }
        x = wave_scan(x, lane);
        if (i < N) W.map[v] = carry + x - 1;
        carry += __shfl(x, 63, 64);
    }
    return carry;
}

template <uint32_t PH>
__global__ __launch_bounds__(64) void k_lg_msa(LArgs a) {
    const uint32_t lane = threadIdx.x;
    if constexpr (PH == 0) {
        LWin& W = a.win[blockIdx.x];
        if (W.phase != PH_DONE || W.grow || W.status != VC_WIN_OK) return;
        const LGraph& g = W.gr[W.cur];
        if (!(a.msa & VC_POA_MSA)) return;
        const uint32_t cols = msa_columns(W, g, lane);
        if (lane == 0) { W.row_size = cols; W.msa_rows = g.nseq + ((a.msa & VC_POA_MSA_CONSENSUS) ? 1u : 0u); }
    } else {
        LWin& W = a.win[a.list[blockIdx.x]];
        const LGraph& g = W.gr[W.cur];
        uint8_t* out = a.msa_out + a.hoff[blockIdx.x];                     // 16-byte aligned
        const uint64_t rs = W.row_size, total = (uint64_t)W.msa_rows * rs;
        const uint32_t fill = 0x2D2D2D2Du;                                 // '-'
        uint4* o4 = (uint4*)out;
        for (uint64_t k = lane; k < total / 16; k += 64) o4[k] = make_uint4(fill, fill, fill, fill);
        for (uint64_t k = (total & ~15ull) + lane; k < total; k += 64) out[k] = '-';
        __syncthreads();
        if (total) {
            for (uint32_t s = lane; s < g.nseq; s += 64) {
                const uint32_t v = W.sq_begin[s];
                out[(uint64_t)s * rs + W.map[v]] = (uint8_t)W.decoder[g.code[v]];
            }
            for (uint32_t e = lane; e < g.n_edges; e += 64) {
                const uint32_t h = g.head[e];
                const uint64_t col = W.map[h];
                const uint8_t ch = (uint8_t)W.decoder[g.code[h]];
                for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) out[(uint64_t)g.lb_v[c] * rs + col] = ch;
            }
            if (a.msa & VC_POA_MSA_CONSENSUS) {
                uint8_t* row = out + (uint64_t)g.nseq * rs;
                for (uint32_t i = lane; i < W.cons_n; i += 64) row[W.map[W.comp[i]]] = W.cons[i];
            }
        }
        uint32_t* mem = (uint32_t*)(out + ((total + 15) & ~15ull));
        for (uint32_t s = lane; s < W.msa_rows; s += 64) mem[s] = s < g.nseq ? W.sq_member[s] : VC_POA_ROW_CONSENSUS;
        if (a.msa & VC_POA_COVERAGE) {
            uint32_t* cov = mem + ((W.msa_rows + 3) & ~3u);
            for (uint32_t i = lane; i < W.cons_n; i += 64) {
                const uint32_t v = W.comp[i];
                uint32_t cnt = 0, u = v;
                for (uint32_t q = g.al_h[v];; q = g.al_nx[q]) {           // the node, then its aligned nodes
                    for (uint32_t e = g.in_h[u]; e != NONE; e = g.nx_in[e])
                        for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) cnt++;
                    for (uint32_t e = g.out_h[u]; e != NONE; e = g.nx_out[e])
                        for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) cnt += W.sq_begin[g.lb_v[c]] == u;
                    if (q == NONE) break;
                    u = g.al_v[q];
                }
                cov[i] = cnt;
            }
        }
    }
}

// A finished group's block of k_lg_graph<1>: the byte offset of every table in it, each 16-byte aligned and padded to 16 bytes
// (the fills store whole uint4).  N nodes, E edges, P aligned pairs, S added sequences, T path entries, C consensus nodes.
struct GraphBlock {
    uint64_t base, cons_pos, rank, out_off, head, weight, al_a, al_b, member, rev, p_off, p_node, cons_node, bytes;
};
__host__ __device__ inline GraphBlock graph_block(uint64_t N, uint64_t E, uint64_t P, uint64_t S, uint64_t T, uint64_t Cn) {
    GraphBlock B;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = off; off += (bytes + 15) & ~15ull; return at; };
    B.base = take(N); B.cons_pos = take(4 * N); B.rank = take(4 * N); B.out_off = take(4 * (N + 1));
    B.head = take(4 * E); B.weight = take(8 * E);
    B.al_a = take(4 * P); B.al_b = take(4 * P);
    B.member = take(4 * S); B.rev = take(S); B.p_off = take(4 * (S + 1)); B.p_node = take(4 * T);
    B.cons_node = take(4 * Cn);
    B.bytes = off;
    return B;
}
// the (sequence, column) scratch of the path stage beside it
__host__ __device__ inline uint64_t graph_scratch_bytes(uint64_t S, uint64_t cols) { return (4 * S * cols + 15) & ~15ull; }

// The partial order graph of a finished POA group, as spoa's PrintGfa (main.cpp:120-200) and Graph::PrintDot (graph.cpp:746-803)
// read it: one wave per group, no lane-serial stage.  Node ids are the table index, which is spoa's id: add_node numbers the
// nodes in creation order and schedule 2 never rebuilds its graph.
//   PH 0, every group in flight: what PH 1 writes, for the host to size and place the block.  Nodes n_nodes; edges n_edges (every
//     edge lies in exactly one out-list and schedule 2 removes none); aligned pairs n_al / 2 (push_aligned always stores a pair
//     both ways); the columns of the alignment (msa_columns) into W.gr_cols; the path entries -- a path has a node per base, so
//     the lengths of the added sequences, summed over the wave -- into W.gr_path.
//   PH 1, the groups of a.list, block at a.msa_out + a.hoff[blockIdx.x] (graph_block), scratch at a.hoff[groups + blockIdx.x]:
//     per node its base, its consensus position (filled with -1, then scattered from the bundle W.comp) and rank_to_node;
//     out-edges as CSR by tail id and out-list position: a wave prefix sum of out_n over tiles of 64 nodes with a carried
//     total, then every lane walks its own node's list into its slots; the aligned pairs (a, b), a < b, the same way on the
//     count of larger ids in a's aligned list; a path per added sequence.  PrintGfa walks Successor(i) from sequences_[i]; as in
//     k_lg_msa<1> the nodes of sequence i are its begin node and the head of every edge that carries label i, each met once, and
//     an edge goes from a column to a later one, so the path is those nodes in column order: they are scattered into row i of
//     the scratch (S x columns of NONE) and every row is compacted with a wave prefix sum behind the sequence's offset (a
//     prefix sum of the lengths).  a.graph == 2 takes the literal walk instead, a lane per sequence: the dependent chain, kept
//     to be measured against.  A kept reverse strand's path stays in graph order and is flagged (main.cpp:178-187 reverses it
//     while printing).
template <uint32_t PH>
__global__ __launch_bounds__(64) void k_lg_graph(LArgs a) {
    const uint32_t lane = threadIdx.x;
    if constexpr (PH == 0) {
        LWin& W = a.win[blockIdx.x];
        if (W.phase != PH_DONE || W.grow || W.status != VC_WIN_OK) return;
        const LGraph& g = W.gr[W.cur];
        const uint32_t cols = msa_columns(W, g, lane);
        uint32_t t = 0;
        for (uint32_t s = lane; s < g.nseq; s += 64) {
            const uint32_t q = W.s0 + W.sq_member[s];
            t += (uint32_t)(a.seq_off[q + 1] - a.seq_off[q]);
        }
        for (uint32_t d = 32; d; d >>= 1) t += __shfl_xor(t, d, 64);
        if (lane == 0) { W.gr_cols = cols; W.gr_path = t; }
    } else {
        LWin& W = a.win[a.list[blockIdx.x]];
        const LGraph& g = W.gr[W.cur];
        const uint32_t N = g.n_nodes, E = g.n_edges, P = g.n_al / 2, S = g.nseq, T = W.gr_path, Cn = W.cons_n, cols = W.gr_cols;
        const GraphBlock B = graph_block(N, E, P, S, T, Cn);
        uint8_t* out = a.msa_out + a.hoff[blockIdx.x];                     // 16-byte aligned, and so is every table
        uint8_t* base = out + B.base;
        int32_t* cons_pos = (int32_t*)(out + B.cons_pos);
        uint32_t *rank = (uint32_t*)(out + B.rank), *out_off = (uint32_t*)(out + B.out_off), *head = (uint32_t*)(out + B.head);
        int64_t* weight = (int64_t*)(out + B.weight);
        uint32_t *al_a = (uint32_t*)(out + B.al_a), *al_b = (uint32_t*)(out + B.al_b), *member = (uint32_t*)(out + B.member);
        uint8_t* rev = out + B.rev;
        uint32_t *p_off = (uint32_t*)(out + B.p_off), *p_node = (uint32_t*)(out + B.p_node), *cons_node = (uint32_t*)(out + B.cons_node);
        uint32_t* scr = (uint32_t*)(a.msa_out + a.hoff[gridDim.x + blockIdx.x]);
        const uint64_t cells = a.graph == 1 ? (uint64_t)S * cols : 0;
        const uint4 none4 = make_uint4(NONE, NONE, NONE, NONE);
        for (uint64_t k = lane; k < ((uint64_t)N + 3) / 4; k += 64) ((uint4*)cons_pos)[k] = none4;      // -1
        for (uint64_t k = lane; k < (cells + 3) / 4; k += 64) ((uint4*)scr)[k] = none4;
        for (uint32_t v = lane; v < N; v += 64) { base[v] = (uint8_t)W.decoder[g.code[v]]; rank[v] = g.rank[v]; }
        // the sequences: member, strand, offset of the path
        uint32_t carry = 0;
        for (uint32_t s0 = 0; s0 < S; s0 += 64) {
            const uint32_t s = s0 + lane;
            uint32_t len = 0;
            if (s < S) {
                const uint32_t q = W.s0 + W.sq_member[s];
                len = (uint32_t)(a.seq_off[q + 1] - a.seq_off[q]);
                member[s] = W.sq_member[s];
                rev[s] = a.strand ? a.s_rev[q] : 0;
            }
            const uint32_t x = wave_scan(len, lane);
            if (s < S) p_off[s] = carry + x - len;
            carry += __shfl(x, 63, 64);
        }
        if (lane == 0) p_off[S] = carry;
        __syncthreads();
        for (uint32_t i = lane; i < Cn; i += 64) { cons_pos[W.comp[i]] = (int32_t)i; cons_node[i] = W.comp[i]; }
        // out-edges and aligned pairs
        uint32_t ce = 0, cp = 0;
        for (uint32_t v0 = 0; v0 < N; v0 += 64) {
            const uint32_t v = v0 + lane;
            uint32_t ne = 0, np = 0;
            if (v < N) {
                ne = g.out_n[v];
                for (uint32_t q = g.al_h[v]; q != NONE; q = g.al_nx[q]) np += g.al_v[q] > v;
            }
            const uint32_t xe = wave_scan(ne, lane), xp = wave_scan(np, lane);
            if (v < N) {
                uint32_t k = ce + xe - ne;
                out_off[v] = k;
                for (uint32_t e = g.out_h[v]; e != NONE && k < E; e = g.nx_out[e], ++k) { head[k] = g.head[e]; weight[k] = g.weight[e]; }
                k = cp + xp - np;
                for (uint32_t q = g.al_h[v]; q != NONE; q = g.al_nx[q])
                    if (g.al_v[q] > v && k < P) { al_a[k] = v; al_b[k] = g.al_v[q]; ++k; }
            }
            ce += __shfl(xe, 63, 64); cp += __shfl(xp, 63, 64);
        }
        if (lane == 0) out_off[N] = ce;
        // the paths
        if (a.graph == 2) {
            for (uint32_t s = lane; s < S; s += 64) {
                uint32_t k = p_off[s];
                const uint32_t end = p_off[s + 1];
                for (uint32_t v = W.sq_begin[s]; v != NONE && k < end;) {
                    p_node[k++] = v;
                    uint32_t nx = NONE;                                    // Node::Successor, graph.cpp:28-39
                    for (uint32_t e = g.out_h[v]; e != NONE && nx == NONE; e = g.nx_out[e])
                        for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) if (g.lb_v[c] == s) { nx = g.head[e]; break; }
                    v = nx;
                }
            }
            return;
        }
        for (uint32_t s = lane; s < S; s += 64) {
            const uint32_t v = W.sq_begin[s];
            scr[(uint64_t)s * cols + W.map[v]] = v;
        }
        for (uint32_t e = lane; e < E; e += 64) {
            const uint32_t h = g.head[e];
            const uint64_t col = W.map[h];
            for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) scr[(uint64_t)g.lb_v[c] * cols + col] = h;
        }
        __syncthreads();
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t* row = scr + (uint64_t)s * cols;
            const uint32_t end = p_off[s + 1];
            uint32_t at = p_off[s];
            for (uint32_t c0 = 0; c0 < cols; c0 += 64) {
                const uint32_t v = c0 + lane < cols ? row[c0 + lane] : NONE;
                const uint32_t x = wave_scan(v != NONE, lane);
                if (v != NONE && at + x - 1 < end) p_node[at + x - 1] = v;
                at += __shfl(x, 63, 64);
            }
        }
    }
}

// ------------------------------------------------------------------ host
thread_local std::string g_err;
int fail(int rc, const char* m) { g_err = m; return rc; }

struct Caps { uint64_t NC, EC, AC, LC, SC, PC, nseq; };

// bytes of a window's tables, and (base != nullptr) the pointers into them
uint64_t layout(LWin* W, uint8_t* base, const Caps& c, bool labels, bool msa) {
    uint64_t off = 0;
    auto take = [&](auto** p, uint64_t n) {
        using T = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
        off = (off + 15) & ~15ull;
        if (base) *p = (T)(base + off);
        off += n * sizeof(**p);
    };
    LWin tmp{};
    LWin* x = base ? W : &tmp;
    for (int k = 0; k < 2; ++k) {
        LGraph& g = x->gr[k];
        take(&g.code, c.NC);
        for (uint32_t** p : {&g.in_h, &g.in_t, &g.in_n, &g.out_h, &g.out_t, &g.out_n, &g.al_h, &g.al_t, &g.al_n, &g.rank}) take(p, c.NC);
        for (uint32_t** p : {&g.tail, &g.head, &g.nx_in, &g.nx_out, &g.lb_h, &g.lb_t}) take(p, c.EC);
        take(&g.weight, c.EC);
        take(&g.alive, c.EC);
        take(&g.al_v, c.AC); take(&g.al_nx, c.AC);
        const uint64_t lc = (k == 0 && labels) ? c.LC : 1;
        take(&g.lb_v, lc); take(&g.lb_nx, lc);
    }
    take(&x->coder, 256); take(&x->decoder, 256);
    take(&x->mark, c.NC); take(&x->ign, c.NC);
    take(&x->stack, c.SC);
    for (uint32_t** p : {&x->node_rank, &x->map, &x->g2s, &x->fr_v, &x->fr_e, &x->comp, &x->best, &x->pred}) take(p, c.NC);
    take(&x->stamp, c.nseq + 1);
    take(&x->fr_p, c.NC);
    take(&x->scores, c.NC);
    take(&x->rchar, c.NC); take(&x->sink, c.NC);
    take(&x->poff, c.NC + 1); take(&x->prank, c.EC);
    take(&x->pairs, 2 * c.PC);
    take(&x->cons, c.NC);
    if (msa) { take(&x->sq_begin, c.nseq); take(&x->sq_member, c.nseq); }
    return (off + 255) & ~255ull;
}

// device buffers kept between calls (grow-only, one device) and given back by vc_large_release()
struct Buf { void* p = nullptr; uint64_t bytes = 0; };
struct Cache { int device = -1; Buf arena, mat; } g_cache;

void* cached(Buf& b, uint64_t bytes) {
    if (b.p && b.bytes >= bytes) return b.p;
    if (b.p) { (void)hipFree(b.p); b = Buf{}; }
    if (hipMalloc(&b.p, std::max<uint64_t>(bytes, 256)) != hipSuccess) { (void)hipGetLastError(); b = Buf{}; return nullptr; }
    b.bytes = std::max<uint64_t>(bytes, 256);
    return b.p;
}

void release_cache() {
    if (g_cache.device >= 0) (void)hipSetDevice(g_cache.device);
    if (g_cache.arena.p) (void)hipFree(g_cache.arena.p);
    if (g_cache.mat.p) (void)hipFree(g_cache.mat.p);
    g_cache = Cache{};
}

// the device allocations of one scope, freed when it ends
struct DevMem {
    std::vector<void*> held;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { for (void* q : held) (void)hipFree(q); }
    // n elements (at least one), filled from src where there is one
    template <class T> bool alloc(T** p, size_t n, const void* src = nullptr) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
        held.push_back(q);
        *p = (T*)q;
        return !src || n == 0 || hipMemcpy(q, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
};

// the development knobs of the header comment; false: VC_LARGE_CAPS does not parse
constexpr char kTables[] = "nealsp";                   // Knobs::shift order
struct Knobs { uint32_t shift[6] = {0, 0, 0, 0, 0, 0}; uint64_t arena = 0, mat = 0; bool log = false; };

bool read_knobs(Knobs& k) {
    k = Knobs{};
    auto mib = [](const char* name) -> uint64_t {
        const char* v = getenv(name);
        const double x = v ? std::atof(v) : 0.0;
        return x > 0 ? std::max<uint64_t>((uint64_t)(x * 1048576.0), 1) : 0;
    };
    k.arena = mib("VC_LARGE_ARENA_MB");
    k.mat = mib("VC_LARGE_MAT_MB");
    const char* lg = getenv("VC_LARGE_LOG");
    k.log = lg && std::atoi(lg) != 0;
    const char* c = getenv("VC_LARGE_CAPS");
    if (!c) return true;
    while (*c) {
        const char* t = std::strchr(kTables, *c);
        if (!t || c[1] != ':') return false;
        char* end = nullptr;
        const long s = std::strtol(c + 2, &end, 10);
        if (end == c + 2 || s < 0 || s > 40) return false;
        k.shift[t - kTables] = (uint32_t)s;
        c = end;
        if (*c == ',') ++c;
        else if (*c) return false;
    }
    return true;
}

// LArgs::graph of vc_poa_run_graph: 1, or 2 with VC_LARGE_GRAPH_WALK=1 (the paths by the literal walk: only to be measured)
uint32_t graph_route() {
    const char* v = getenv("VC_LARGE_GRAPH_WALK");
    return v && std::atoi(v) != 0 ? 2 : 1;
}

uint64_t shrunk(uint64_t v, uint32_t s) { return std::max<uint64_t>(v >> s, 1); }

// initial tables of a window or group from its sum of sequence lengths and its longest sequence.  Nodes: every node is made from
// one base of one sequence, so the sum bounds them; the rest starts from what such graphs use and doubles when a table fills.
Caps initial_caps(uint64_t sum, uint64_t mx, uint64_t nseq, const Knobs& kn) {
    Caps c;
    c.NC = sum + 1; c.EC = sum + 64; c.AC = 2 * sum + 64; c.LC = sum + 64; c.SC = c.NC + c.EC + c.AC; c.PC = sum + mx + 2;
    c.nseq = nseq;
    c.NC = shrunk(c.NC, kn.shift[0]); c.EC = shrunk(c.EC, kn.shift[1]); c.AC = shrunk(c.AC, kn.shift[2]);
    c.LC = shrunk(c.LC, kn.shift[3]); c.SC = shrunk(c.SC, kn.shift[4]); c.PC = shrunk(c.PC, kn.shift[5]);
    return c;
}

// VC_OK, or the error of a device the kernels cannot run on
int check_device(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(VC_ERR_NO_DEVICE, "no HIP device visible; the large-graph path has no CPU fallback");
    }
    if (device < 0 || device >= ndev) return fail(VC_ERR_NO_DEVICE, "no HIP device with this ordinal");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(VC_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(VC_ERR_NO_DEVICE, "the kernels are built for gfx950 only");
    return VC_OK;
}

// what vc_poa_run_msa hands out: owned here, valid until the next vc_poa_* / vc_large_* call or vc_large_release
struct MsaStore {
    std::vector<uint32_t> n_rows, row_size, row_member, coverage;
    std::vector<uint64_t> row_off, member_off;
    std::vector<uint8_t> rows;
    void clear() { *this = MsaStore{}; }
} g_msa;

// what vc_poa_run_graph hands out, with the same lifetime: the tables of vc_poa_graph_out
struct GraphStore {
    std::vector<uint32_t> n_nodes, rank_to_node, edge_head, aligned_a, aligned_b, path_member, path_node, cons_node;
    std::vector<uint64_t> node_off, out_off, aligned_off, path_first, path_off;
    std::vector<uint8_t> node_base, path_reversed;
    std::vector<int32_t> node_cons_pos;
    std::vector<int64_t> edge_weight;
    uint64_t bytes = 0;                                // copied out of the device
    void clear() { *this = GraphStore{}; }
} g_graph;

// what vc_poa_run_align hands out, with the same lifetime: the arrays of vc_poa_align_out, one entry per query of the batch
struct AlignStore {
    std::vector<uint8_t> status, reversed;
    std::vector<int32_t> score, score_rev, pair_node, pair_pos;
    std::vector<uint64_t> pair_off;
    uint64_t bytes = 0;                                // copied out of the device
    void clear() { *this = AlignStore{}; }
} g_align;

// The query stage of one vc_poa_run_align call: the query batch, the flags, and what the stages of the host groups leave -- per
// stage the packed pairs (every node, then every position), per query where its pairs lie -- until assemble puts them in order.
struct AlignReq {
    const vc_batch* q = nullptr;
    uint32_t flags = 0;
    uint64_t nq = 0, nbytes = 0;                       // sequences and bytes of the query batch
    std::vector<std::vector<int32_t>> part;
    std::vector<uint32_t> part_of, count;              // [nq]
    std::vector<uint64_t> first;                       // [nq]
    uint64_t jobs = 0, launches = 0, cells = 0;        // VC_LARGE_LOG's "align" line
};

// a group's block of k_lg_graph<1> on the host, and the counts that lay it out
struct GraphPart { uint32_t N = 0, E = 0, P = 0, S = 0, T = 0, Cn = 0; std::vector<uint8_t> blk; };

// ------------------------------------------------------------------ the host schedule
// One call of vc_large_run / vc_poa_run*: the batch on the device (seq_begin / seq_end only with spans), windows in flight in
// groups that fit the arena budget, one alignment of each per lock-step step with the forward passes in launches that fit the
// matrix budget, and a window whose table filled run again with larger tables.  `a` holds the scores and the schedule.
struct Run {
    LArgs a;
    const vc_batch* b;
    std::vector<Caps>& caps;
    bool labels;
    const Knobs& kn;
    MsaStore* msa;                                     // vc_poa_run_msa with flags, else nullptr
    const vc_poa_strand_out* so;                       // vc_poa_run_strand, else nullptr
    uint32_t nw;
    uint64_t nseq_all, nbytes;
    uint64_t arena_budget = 0, mat_budget = 0;
    uint64_t planes = 1;                               // int32 planes per matrix cell
    uint32_t ns = 1;                                   // forward passes, and matrices, per alignment: one per strand
    std::vector<uint32_t> pending;                     // windows still to run, in order
    std::vector<std::vector<uint8_t>> out;             // per window: the consensus, ...
    std::vector<uint8_t> status;
    std::vector<std::vector<uint32_t>> mem_of, cov_of; // ... and (msa) row members and coverage
    uint32_t msa_launches = 0;
    uint64_t n_align = 0, n_cells = 0;                 // forward passes run (VC_LARGE_LOG's "done" line)
    GraphStore* gs = nullptr;                          // vc_poa_run_graph, else nullptr
    std::vector<GraphPart> part;                       // ... per window: its block
    uint32_t graph_launches = 0;
    AlignReq* al = nullptr;                            // vc_poa_run_align with queries, else nullptr
    bool seqs() const { return msa != nullptr || gs != nullptr; }   // the windows keep sq_begin / sq_member
};

// the windows in flight together: their ids, their tables in the arena, their LWin here and on the device
struct Group {
    std::vector<uint32_t> ids;
    std::vector<uint64_t> aoff;
    uint64_t abytes = 0;
    std::vector<LWin> hw;
    LWin* d_win = nullptr;
    uint32_t* d_list = nullptr;                        // the windows of one launch (k_lg_fwd / k_lg_back / k_lg_msa<1>) ...
    uint64_t* d_hoff = nullptr;                        // ... and where their matrices or blocks begin
};

int upload_batch(Run& R, DevMem& mem, bool spans) {
    const vc_batch* b = R.b;
    uint32_t lut_w[256];
    double lut_d[256];
    vc_weight_lut(lut_w);
    for (int c = 0; c < 256; ++c) lut_d[c] = 1 - pow(10, (33 - (int)(signed char)c) / 10.0);
    uint64_t* d_so = nullptr; uint32_t *d_sb = nullptr, *d_se = nullptr, *d_lw = nullptr; uint8_t *d_hq = nullptr, *d_b = nullptr, *d_q = nullptr;
    double* d_ld = nullptr;
    if (!mem.alloc(&d_so, R.nseq_all + 1, b->seq_off) ||
        (spans && (!mem.alloc(&d_sb, R.nseq_all, b->seq_begin) || !mem.alloc(&d_se, R.nseq_all, b->seq_end))) ||
        !mem.alloc(&d_hq, R.nseq_all, b->seq_has_qual) || !mem.alloc(&d_b, R.nbytes, b->bases) || !mem.alloc(&d_q, R.nbytes, b->quals) ||
        !mem.alloc(&d_lw, 256, lut_w) || !mem.alloc(&d_ld, 256, lut_d))
        return fail(VC_ERR_HIP, "device allocation or copy of the batch failed");
    LArgs& a = R.a;
    a.seq_off = d_so; a.seq_begin = d_sb; a.seq_end = d_se; a.has_qual = d_hq; a.bases = d_b; a.quals = d_q; a.lut_w = d_lw; a.lut_d = d_ld;
    return VC_OK;
}

// vc_poa_run_strand: the strand views, once per call, and the zeroed choices
int strand_views(Run& R, DevMem& mem) {
    LArgs& a = R.a;
    const uint64_t nseq_all = R.nseq_all, nbytes = R.nbytes;
    a.nbytes = nbytes;
    bool ok = mem.alloc(&a.rc_bases, nbytes) && mem.alloc(&a.rv_quals, nbytes) && mem.alloc(&a.rt_bases, nbytes) &&
              mem.alloc(&a.s_rev, nseq_all) && mem.alloc(&a.s_score, nseq_all) && mem.alloc(&a.s_score_rev, nseq_all) &&
              hipMemset(a.s_rev, 0, std::max<size_t>(nseq_all, 1)) == hipSuccess &&
              hipMemset(a.s_score, 0, std::max<size_t>(nseq_all, 1) * 4) == hipSuccess &&
              hipMemset(a.s_score_rev, 0, std::max<size_t>(nseq_all, 1) * 4) == hipSuccess;
    if (ok && nbytes) {
        hipLaunchKernelGGL(k_lg_views, dim3((uint32_t)((nbytes + 255) / 256)), dim3(256), 0, 0, a, (uint32_t)nseq_all);
        ok = hipGetLastError() == hipSuccess;
    }
    return ok ? VC_OK : fail(VC_ERR_HIP, "device allocation or launch of the strand views failed");
}

// vc_poa_run_align: the query batch on the device -- offsets and bytes, and with VC_POA_ALIGN_STRANDS its reverse-complement
// view (k_lg_views on the query batch's arrays: no quality, no round trip) -- once per call
int upload_queries(Run& R, DevMem& mem) {
    AlignReq& A = *R.al;
    uint64_t* d_off = nullptr;
    uint8_t *d_b = nullptr, *d_rc = nullptr;
    const bool strands = (A.flags & VC_POA_ALIGN_STRANDS) != 0;
    bool ok = mem.alloc(&d_off, A.nq + 1, A.q->seq_off) && mem.alloc(&d_b, A.nbytes, A.q->bases) && (!strands || mem.alloc(&d_rc, A.nbytes));
    if (ok && strands && A.nbytes) {
        LArgs v{};
        v.seq_off = d_off; v.bases = d_b; v.rc_bases = d_rc; v.nbytes = A.nbytes;
        hipLaunchKernelGGL(k_lg_views, dim3((uint32_t)((A.nbytes + 255) / 256)), dim3(256), 0, 0, v, (uint32_t)A.nq);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) return fail(VC_ERR_HIP, "device allocation, copy or strand view of the query batch failed");
    R.a.q_off = d_off; R.a.q_bases = d_b; R.a.q_rc = d_rc;
    return VC_OK;
}

// The windows in flight next: as many of the pending ones as the arena budget holds, in order (at least one; a window the device
// cannot hold at all is refused).  G.ids is empty when every pending window was refused.
void next_group(Run& R, Group& G) {
    std::vector<uint32_t> rest;
    for (uint32_t w : R.pending) {
        const uint64_t need = layout(nullptr, nullptr, R.caps[w], R.labels, R.seqs());
        if (G.ids.empty() && need > R.arena_budget * 2) {                  // the device cannot hold its tables
            R.status[w] = VC_WIN_OVERFLOW;
            if (R.kn.log) std::fprintf(stderr, "vc_large: refuse window=%u bytes=%llu budget=%llu\n", w, (unsigned long long)need, (unsigned long long)R.arena_budget);
            continue;
        }
        if (!G.ids.empty() && G.abytes + need > R.arena_budget) { rest.push_back(w); continue; }
        G.ids.push_back(w); G.aoff.push_back(G.abytes); G.abytes += need;
    }
    R.pending.swap(rest);
    const uint32_t n = (uint32_t)G.ids.size();
    if (!R.kn.log || n == 0) return;
    std::string ids, needs;
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t end = k + 1 < n ? G.aoff[k + 1] : G.abytes;
        ids += (k ? "," : "") + std::to_string(G.ids[k]);
        needs += (k ? "," : "") + std::to_string(end - G.aoff[k]);
    }
    std::fprintf(stderr, "vc_large: group windows=%u bytes=%llu ids=%s need=%s\n", n, (unsigned long long)G.abytes, ids.c_str(), needs.c_str());
}

// the group's LWin on the host: tables in the arena, the window's sequences and capacities
void place_windows(const Run& R, Group& G, uint8_t* arena) {
    const vc_batch* b = R.b;
    G.hw.resize(G.ids.size());
    for (size_t k = 0; k < G.ids.size(); ++k) {
        const uint32_t w = G.ids[k];
        LWin& W = G.hw[k];
        W = LWin{};
        layout(&W, arena + G.aoff[k], R.caps[w], R.labels, R.seqs());
        const Caps& c = R.caps[w];
        W.s0 = b->win_seq_off[w]; W.nseq = b->win_seq_off[w + 1] - W.s0;
        W.L = W.nseq ? (uint32_t)(b->seq_off[W.s0 + 1] - b->seq_off[W.s0]) : 0;     // (POA groups: unused, and may be empty)
        W.fasta = b->win_fasta && b->win_fasta[w] ? 1 : 0;
        W.NC = (uint32_t)c.NC; W.EC = (uint32_t)c.EC; W.AC = (uint32_t)c.AC; W.LC = (uint32_t)c.LC; W.SC = (uint32_t)c.SC; W.PC = (uint32_t)c.PC;
    }
}

// The next launch over items[k0 ..): consecutive items while their sizes fit the budget -- at least one, however large.  list and
// off (where each item begins) describe it, total is its size; returns the first item left for the launch after.
template <class Size>
size_t pack_launch(const std::vector<uint32_t>& items, size_t k0, uint64_t budget, Size size, std::vector<uint32_t>& list,
                   std::vector<uint64_t>& off, uint64_t& total) {
    list.clear(); off.clear(); total = 0;
    for (; k0 < items.size(); ++k0) {
        const uint64_t need = size(items[k0]);
        if (!list.empty() && total + need > budget) break;
        list.push_back(items[k0]); off.push_back(total); total += need;
    }
    return k0;
}

bool upload_launch(const Group& G, const std::vector<uint32_t>& list, const std::vector<uint64_t>& off) {
    return hipMemcpy(G.d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemcpy(G.d_hoff, off.data(), off.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
}

template <uint32_t GM>
void launch_align(const LArgs& f, uint32_t nl, uint32_t ns) {
    hipLaunchKernelGGL(k_lg_fwd<GM>, dim3(nl, ns), dim3(64), 0, 0, f);
    hipLaunchKernelGGL(k_lg_back<GM>, dim3((nl + 63) / 64), dim3(64), 0, 0, f, nl);
}

// The forward passes and backtracks of one step, over the windows `act` that have an alignment: their matrices in launches that
// fit the budget (in int32 cells of every plane and strand); a matrix the device cannot hold takes its window out.
bool align_step(Run& R, Group& G, const std::vector<uint32_t>& act) {
    uint32_t launches = 0, over = 0;
    std::vector<uint32_t> list;
    std::vector<uint64_t> hoff;
    auto matrix_cells = [&](uint32_t k) { return ((uint64_t)G.hw[k].rows + 1) * ((uint64_t)G.hw[k].qlen + 1) * R.planes * R.ns; };
    for (size_t k0 = 0; k0 < act.size();) {
        uint64_t cells;
        k0 = pack_launch(act, k0, R.mat_budget / 4, matrix_cells, list, hoff, cells);
        int32_t* H = (int32_t*)cached(g_cache.mat, cells * 4);
        if (!H) {
            if (list.size() > 1) return false;
            LWin& W = G.hw[list[0]];
            W.phase = PH_DONE; W.status = VC_WIN_OVERFLOW; W.rows = 0;
            if (hipMemcpy(G.d_win + list[0], &W, sizeof(LWin), hipMemcpyHostToDevice) != hipSuccess) return false;
            continue;
        }
        if (!upload_launch(G, list, hoff)) return false;
        const uint32_t nl = (uint32_t)list.size();
        LArgs f = R.a;
        f.list = G.d_list; f.hoff = G.d_hoff; f.H = H;
        if (f.gaps == 0) launch_align<0>(f, nl, R.ns);
        else if (f.gaps == 1) launch_align<1>(f, nl, R.ns);
        else launch_align<2>(f, nl, R.ns);
        const bool ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        for (const uint32_t k : list) R.n_cells += (uint64_t)G.hw[k].rows * G.hw[k].qlen * R.ns;
        R.n_align += (uint64_t)nl * R.ns;
        launches++;
        if (cells * 4 > R.mat_budget) over++;
        if (!ok) return false;
    }
    if (R.kn.log && launches > 1) std::fprintf(stderr, "vc_large: step launches=%u over=%u\n", launches, over);
    return true;
}

// The lock-step schedule of one group: one alignment of every window in flight per step, until none is live; then (msa) columns,
// row_size and rows of every finished group.  G.hw holds the windows' final state.
bool lock_step(Run& R, Group& G) {
    const LArgs& a = R.a;
    const uint32_t n = (uint32_t)G.ids.size();
    const dim3 lanes((n + 63) / 64);
    bool ok = hipMemcpy(G.d_win, G.hw.data(), n * sizeof(LWin), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { hipLaunchKernelGGL(k_lg_init, lanes, dim3(64), 0, 0, a); ok = hipGetLastError() == hipSuccess; }
    while (ok) {
        hipLaunchKernelGGL(k_lg_prep, lanes, dim3(64), 0, 0, a);
        if (hipMemcpy(G.hw.data(), G.d_win, n * sizeof(LWin), hipMemcpyDeviceToHost) != hipSuccess) return false;
        bool live = false;
        std::vector<uint32_t> act;
        for (uint32_t k = 0; k < n; ++k) {
            if (G.hw[k].phase != PH_DONE && !G.hw[k].grow) live = true;
            if (G.hw[k].rows) act.push_back(k);
        }
        if (!live) break;
        if (!align_step(R, G, act)) return false;
        hipLaunchKernelGGL(k_lg_apply, lanes, dim3(64), 0, 0, a);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && R.msa) {
        hipLaunchKernelGGL(k_lg_msa<0>, dim3(n), dim3(64), 0, 0, a);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && R.gs) {
        hipLaunchKernelGGL(k_lg_graph<0>, dim3(n), dim3(64), 0, 0, a);
        ok = hipGetLastError() == hipSuccess;
    }
    return ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(G.hw.data(), G.d_win, n * sizeof(LWin), hipMemcpyDeviceToHost) == hipSuccess;
}

// a table of window w filled (W.grow): larger tables, and the window runs again unless they outgrow the 32-bit ids
void regrow(Run& R, uint32_t w, const LWin& W) {
    Caps& c = R.caps[w];
    if (W.grow & G_NODES) c.NC *= 2;
    if (W.grow & G_EDGES) c.EC *= 2;
    if (W.grow & G_ALIGNED) c.AC *= 2;
    if (W.grow & G_LABELS) c.LC *= 2;
    if (W.grow & G_PAIRS) c.PC *= 2;
    c.SC = std::max<uint64_t>(c.SC * ((W.grow & G_STACK) ? 2 : 1), (c.NC + c.EC + c.AC) >> R.kn.shift[4]);
    if (R.kn.log) {
        std::string fl;
        static const char* const names[] = {"nodes", "edges", "aligned", "labels", "stack", "pairs"};
        for (int t = 0; t < 6; ++t) if (W.grow & (1u << t)) { if (!fl.empty()) fl += ','; fl += names[t]; }
        std::fprintf(stderr, "vc_large: regrow window=%u flags=%s caps n=%llu e=%llu a=%llu l=%llu s=%llu p=%llu\n", w, fl.c_str(),
                     (unsigned long long)c.NC, (unsigned long long)c.EC, (unsigned long long)c.AC, (unsigned long long)c.LC,
                     (unsigned long long)c.SC, (unsigned long long)c.PC);
    }
    if (c.NC >= (1ull << 31) || c.EC >= (1ull << 31) || c.AC >= (1ull << 31) || c.SC >= (1ull << 31) || c.PC >= (1ull << 30))
        R.status[w] = VC_WIN_OVERFLOW;
    else
        R.pending.push_back(w);
}

// A finished group's block of k_lg_msa<1>: msa_rows x row_size bytes, then (16-byte aligned) the row members at mem_at, then
// (16-byte aligned, VC_POA_COVERAGE) the coverage at cov_at.
struct MsaBlock { uint64_t mem_at, cov_at, bytes; };
MsaBlock msa_block(const LWin& W, uint32_t flags) {
    MsaBlock B;
    B.mem_at = ((uint64_t)W.msa_rows * W.row_size + 15) & ~15ull;
    B.cov_at = B.mem_at + 4 * (((uint64_t)W.msa_rows + 3) & ~3ull);
    B.bytes = B.cov_at + ((flags & VC_POA_COVERAGE) ? 4 * (((uint64_t)W.cons_n + 3) & ~3ull) : 0);
    return B;
}

// The alignments and coverage of the groups that finished, while their tables are resident: blocks laid out in the matrix buffer
// (free after the last step), in launches that fit the matrix budget, each copied out at once.
int collect_msa(Run& R, Group& G) {
    const LArgs& a = R.a;
    MsaStore* msa = R.msa;
    std::vector<uint32_t> fin, list;
    std::vector<uint64_t> hoff;
    for (uint32_t k = 0; k < G.ids.size(); ++k) if (!G.hw[k].grow && G.hw[k].status == VC_WIN_OK) fin.push_back(k);
    auto block_bytes = [&](uint32_t k) { return msa_block(G.hw[k], a.msa).bytes; };
    for (size_t k0 = 0; k0 < fin.size();) {
        uint64_t bytes;
        k0 = pack_launch(fin, k0, R.mat_budget, block_bytes, list, hoff, bytes);
        uint8_t* dout = (uint8_t*)cached(g_cache.mat, bytes);
        if (!dout) {
            if (list.size() > 1) return fail(VC_ERR_HIP, "device allocation of the alignment rows failed");
            R.status[G.ids[list[0]]] = VC_WIN_OVERFLOW; R.out[G.ids[list[0]]].clear();
            continue;
        }
        const uint32_t nl = (uint32_t)list.size();
        const uint64_t at = msa->rows.size();
        LArgs f = a;
        f.list = G.d_list; f.hoff = G.d_hoff; f.msa_out = dout;
        bool ok = upload_launch(G, list, hoff);
        if (ok) {
            hipLaunchKernelGGL(k_lg_msa<1>, dim3(nl), dim3(64), 0, 0, f);
            ok = hipGetLastError() == hipSuccess;
            msa->rows.resize(at + bytes);
            ok = ok && hipMemcpy(msa->rows.data() + at, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (!ok) return fail(VC_ERR_HIP, "the alignment-row kernel or its copy failed");
        for (uint32_t q = 0; q < nl; ++q) {
            const LWin& W = G.hw[list[q]];
            const uint32_t w = G.ids[list[q]];
            const MsaBlock B = msa_block(W, a.msa);
            const uint8_t* blk = msa->rows.data() + at + hoff[q];
            msa->n_rows[w] = W.msa_rows; msa->row_size[w] = W.row_size; msa->row_off[w] = at + hoff[q];
            R.mem_of[w].resize(W.msa_rows);
            if (W.msa_rows) std::memcpy(R.mem_of[w].data(), blk + B.mem_at, 4ull * W.msa_rows);
            if (a.msa & VC_POA_COVERAGE) {
                R.cov_of[w].resize(W.cons_n);
                if (W.cons_n) std::memcpy(R.cov_of[w].data(), blk + B.cov_at, 4ull * W.cons_n);
            }
        }
        R.msa_launches++;
    }
    return VC_OK;
}

// The graphs of the groups that finished, as collect_msa: a block and a scratch per group in the matrix buffer, the blocks in
// front so that one copy takes them out and leaves the scratch behind.
int collect_graph(Run& R, Group& G) {
    const LArgs& a = R.a;
    std::vector<uint32_t> fin, list;
    std::vector<uint64_t> hoff;
    for (uint32_t k = 0; k < G.ids.size(); ++k) if (!G.hw[k].grow && G.hw[k].status == VC_WIN_OK && R.status[G.ids[k]] == VC_WIN_OK) fin.push_back(k);
    auto part_of = [&](uint32_t k) {
        const LWin& W = G.hw[k];
        const LGraph& g = W.gr[W.cur];
        GraphPart p;
        p.N = g.n_nodes; p.E = g.n_edges; p.P = g.n_al / 2; p.S = g.nseq; p.T = W.gr_path; p.Cn = W.cons_n;
        return p;
    };
    auto block_of = [&](uint32_t k) { const GraphPart p = part_of(k); return graph_block(p.N, p.E, p.P, p.S, p.T, p.Cn).bytes; };
    auto scratch_of = [&](uint32_t k) { return a.graph == 1 ? graph_scratch_bytes(G.hw[k].gr[G.hw[k].cur].nseq, G.hw[k].gr_cols) : 0; };
    auto need = [&](uint32_t k) { return block_of(k) + scratch_of(k); };
    std::vector<uint8_t> host;
    for (size_t k0 = 0; k0 < fin.size();) {
        uint64_t bytes;
        k0 = pack_launch(fin, k0, R.mat_budget, need, list, hoff, bytes);
        const uint32_t nl = (uint32_t)list.size();
        uint64_t blocks = 0;                                               // every block, then every scratch
        hoff.assign(2 * (size_t)nl, 0);
        for (uint32_t q = 0; q < nl; ++q) { hoff[q] = blocks; blocks += block_of(list[q]); }
        uint64_t at = blocks;
        for (uint32_t q = 0; q < nl; ++q) { hoff[nl + q] = at; at += scratch_of(list[q]); }
        uint8_t* dout = (uint8_t*)cached(g_cache.mat, bytes);
        if (!dout) {
            if (nl > 1) return fail(VC_ERR_HIP, "device allocation of the graph tables failed");
            R.status[G.ids[list[0]]] = VC_WIN_OVERFLOW; R.out[G.ids[list[0]]].clear();
            continue;
        }
        LArgs f = a;
        f.list = G.d_list; f.hoff = G.d_hoff; f.msa_out = dout;
        bool ok = upload_launch(G, list, hoff);
        if (ok) {
            hipLaunchKernelGGL(k_lg_graph<1>, dim3(nl), dim3(64), 0, 0, f);
            ok = hipGetLastError() == hipSuccess;
            host.resize(blocks);
            ok = ok && hipMemcpy(host.data(), dout, blocks, hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (!ok) return fail(VC_ERR_HIP, "the graph kernel or its copy failed");
        for (uint32_t q = 0; q < nl; ++q) {
            GraphPart& p = R.part[G.ids[list[q]]];
            p = part_of(list[q]);
            p.blk.assign(host.begin() + hoff[q], host.begin() + (q + 1 < nl ? hoff[q + 1] : blocks));
        }
        R.gs->bytes += blocks;
        R.graph_launches++;
    }
    return VC_OK;
}

template <uint32_t GM>
void launch_query(const LArgs& f, uint32_t nl, uint32_t ns, bool pairs) {
    hipLaunchKernelGGL(k_lg_qfwd<GM>, dim3(nl, ns), dim3(64), 0, 0, f);
    if (pairs) hipLaunchKernelGGL(k_lg_qback<GM>, dim3((nl + 63) / 64), dim3(64), 0, 0, f, nl);
}

// The query stage of the groups that finished, while their tables are resident (vc_poa_run_align): a job per query, the rows of
// every finished graph once (k_lg_rows), the jobs' forward passes (and, with VC_POA_ALIGN_PAIRS, backtracks) in launches that fit
// the matrix budget -- every (group, query) pair is independent, so a launch holds as many as fit --, the job table back in one
// copy, then the pairs packed behind the host's prefix offsets and out in one copy.
int collect_align(Run& R, Group& G) {
    AlignReq& A = *R.al;
    const LArgs& a = R.a;
    const vc_batch* q = A.q;
    const bool pairs = (A.flags & VC_POA_ALIGN_PAIRS) != 0;
    const uint32_t ns = (A.flags & VC_POA_ALIGN_STRANDS) ? 2 : 1;
    std::vector<LJob> jobs;
    std::vector<uint32_t> act, refused;                                    // jobs with a forward pass; jobs whose matrix the device cannot hold
    uint64_t area = 0;
    for (uint32_t k = 0; k < G.ids.size(); ++k) {
        const LWin& W = G.hw[k];
        const uint32_t w = G.ids[k];
        if (W.grow || W.status != VC_WIN_OK || R.status[w] != VC_WIN_OK) continue;
        const LGraph& g = W.gr[W.cur];
        const uint32_t N = g.n_nodes;
        for (uint32_t s = q->win_seq_off[w]; s < q->win_seq_off[w + 1]; ++s) {
            LJob J{};
            J.win = k; J.qs = s; J.qlen = (uint32_t)(q->seq_off[s + 1] - q->seq_off[s]); J.status = VC_WIN_OK;
            if (N != 0 && J.qlen != 0) {                                   // else an empty alignment, score 0
                // the floor of k_lg_prep, and its check of the topological order
                if (worst_case(a.match, a.gap, a.gap_e, a.gap_q, a.gap_c, (int64_t)J.qlen + 8, N) < (int64_t)KNEG || g.n_rank != N) {
                    J.status = VC_WIN_INVALID;
                } else {
                    J.rows = N; J.area = area;
                    if (pairs) area += (uint64_t)N + J.qlen;
                    act.push_back((uint32_t)jobs.size());
                }
            }
            jobs.push_back(J);
        }
    }
    if (jobs.empty()) return VC_OK;
    A.jobs += jobs.size();
    uint64_t total = 0;
    std::vector<int32_t> packed;
    if (!act.empty()) {
        DevMem mem;
        LJob* d_job = nullptr; uint32_t* d_list = nullptr; uint64_t* d_hoff = nullptr; int32_t *d_pairs = nullptr, *d_out = nullptr;
        if (!mem.alloc(&d_job, jobs.size(), jobs.data()) || !mem.alloc(&d_list, act.size()) || !mem.alloc(&d_hoff, act.size()) ||
            (pairs && !mem.alloc(&d_pairs, 2 * area)))
            return fail(VC_ERR_HIP, "device allocation of the query jobs failed");
        const uint32_t n = (uint32_t)G.ids.size();
        hipLaunchKernelGGL(k_lg_rows, dim3((n + 63) / 64), dim3(64), 0, 0, a);
        if (hipGetLastError() != hipSuccess) return fail(VC_ERR_HIP, "the query stage's row kernel failed");
        std::vector<uint32_t> list;
        std::vector<uint64_t> hoff;
        auto matrix_cells = [&](uint32_t j) { return ((uint64_t)jobs[j].rows + 1) * ((uint64_t)jobs[j].qlen + 1) * R.planes * ns; };
        for (size_t k0 = 0; k0 < act.size();) {
            uint64_t cells;
            k0 = pack_launch(act, k0, R.mat_budget / 4, matrix_cells, list, hoff, cells);
            int32_t* H = (int32_t*)cached(g_cache.mat, cells * 4);
            if (!H) {
                if (list.size() > 1) return fail(VC_ERR_HIP, "device allocation of the query matrices failed");
                refused.push_back(list[0]);
                continue;
            }
            const uint32_t nl = (uint32_t)list.size();
            if (hipMemcpy(d_list, list.data(), nl * 4ull, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_hoff, hoff.data(), nl * 8ull, hipMemcpyHostToDevice) != hipSuccess)
                return fail(VC_ERR_HIP, "copy of a query launch failed");
            LArgs f = a;
            f.job = d_job; f.q_pairs = d_pairs; f.list = d_list; f.hoff = d_hoff; f.H = H;
            if (f.gaps == 0) launch_query<0>(f, nl, ns, pairs);
            else if (f.gaps == 1) launch_query<1>(f, nl, ns, pairs);
            else launch_query<2>(f, nl, ns, pairs);
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(VC_ERR_HIP, "a query kernel failed");
            for (const uint32_t j : list) A.cells += (uint64_t)jobs[j].rows * jobs[j].qlen * ns;
            A.launches++;
        }
        if (hipMemcpy(jobs.data(), d_job, jobs.size() * sizeof(LJob), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VC_ERR_HIP, "copy of the query jobs failed");
        g_align.bytes += jobs.size() * sizeof(LJob);
        for (LJob& J : jobs) { J.pair_off = total; total += J.npairs; }
        if (total) {
            packed.resize(2 * total);
            LArgs f = a;
            f.job = d_job; f.q_pairs = d_pairs;
            bool ok = mem.alloc(&d_out, 2 * total) && hipMemcpy(d_job, jobs.data(), jobs.size() * sizeof(LJob), hipMemcpyHostToDevice) == hipSuccess;
            if (ok) {
                f.q_out = d_out;
                hipLaunchKernelGGL(k_lg_qpack, dim3((uint32_t)jobs.size()), dim3(64), 0, 0, f, total);
                ok = hipGetLastError() == hipSuccess && hipMemcpy(packed.data(), d_out, 8 * total, hipMemcpyDeviceToHost) == hipSuccess;
            }
            if (!ok) return fail(VC_ERR_HIP, "the pack kernel of the query stage or its copy failed");
            g_align.bytes += 8 * total;
        }
    }
    for (const uint32_t j : refused) jobs[j].status = VC_WIN_OVERFLOW;
    AlignStore& S = g_align;
    const uint32_t pi = (uint32_t)A.part.size();
    for (const LJob& J : jobs) {
        const bool ok = J.status == VC_WIN_OK;
        S.status[J.qs] = (uint8_t)J.status;
        S.score[J.qs] = ok ? J.score[0] : 0;
        if (ns == 2) { S.score_rev[J.qs] = ok ? J.score[1] : 0; S.reversed[J.qs] = ok && J.score[0] < J.score[1]; }
        A.part_of[J.qs] = pi; A.first[J.qs] = J.pair_off; A.count[J.qs] = ok ? J.npairs : 0;
    }
    A.part.push_back(std::move(packed));
    return VC_OK;
}

// One group from its tables to its results: a window whose table filled goes back to pending, the others leave their status,
// consensus and (msa) alignment.  A single window the device has no room for is VC_WIN_OVERFLOW; more than one is an error.
int run_group(Run& R, Group& G) {
    const uint32_t n = (uint32_t)G.ids.size();
    uint8_t* arena = (uint8_t*)cached(g_cache.arena, G.abytes);
    DevMem mem;
    if (!arena || !mem.alloc(&G.d_win, n) || !mem.alloc(&G.d_list, n) || !mem.alloc(&G.d_hoff, R.gs ? 2 * (size_t)n : n)) {
        if (n == 1) { R.status[G.ids[0]] = VC_WIN_OVERFLOW; return VC_OK; }
        return fail(VC_ERR_HIP, "device allocation of the window tables failed");
    }
    place_windows(R, G, arena);
    R.a.win = G.d_win; R.a.n = n;
    if (!lock_step(R, G)) return fail(VC_ERR_HIP, "a large-graph kernel failed");
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t w = G.ids[k];
        const LWin& W = G.hw[k];
        if (W.grow) { regrow(R, w, W); continue; }
        R.status[w] = (uint8_t)W.status;
        R.out[w].resize(W.cons_n);
        if (W.cons_n && hipMemcpy(R.out[w].data(), W.cons, W.cons_n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VC_ERR_HIP, "copy of a consensus failed");
    }
    if (R.msa) if (const int rc = collect_msa(R, G)) return rc;
    if (R.gs) if (const int rc = collect_graph(R, G)) return rc;
    return R.al ? collect_align(R, G) : VC_OK;
}

// vc_poa_run_strand: the choices; zeros for the groups that were not computed
int copy_strands(const Run& R) {
    const vc_batch* b = R.b;
    const vc_poa_strand_out* so = R.so;
    bool ok = hipMemcpy(so->reversed, R.a.s_rev, R.nseq_all, hipMemcpyDeviceToHost) == hipSuccess;
    if (so->score) ok = ok && hipMemcpy(so->score, R.a.s_score, R.nseq_all * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (so->score_rev) ok = ok && hipMemcpy(so->score_rev, R.a.s_score_rev, R.nseq_all * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail(VC_ERR_HIP, "copy of the strand choices failed");
    for (uint32_t w = 0; w < R.nw; ++w) {
        if (R.status[w] == VC_WIN_OK) continue;
        for (uint32_t s = b->win_seq_off[w]; s < b->win_seq_off[w + 1]; ++s) {
            so->reversed[s] = 0;
            if (so->score) so->score[s] = 0;
            if (so->score_rev) so->score_rev[s] = 0;
        }
    }
    return VC_OK;
}

// the results in window order: (msa) the per-row and per-base tables, the closing log lines, consensus and status
int assemble(Run& R, vc_result* r) {
    if (MsaStore* msa = R.msa) {
        msa->member_off[0] = 0;
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] != VC_WIN_OK) { msa->n_rows[w] = 0; msa->row_size[w] = 0; R.mem_of[w].clear(); R.cov_of[w].clear(); }
            msa->row_member.insert(msa->row_member.end(), R.mem_of[w].begin(), R.mem_of[w].end());
            msa->member_off[w + 1] = msa->row_member.size();
            if (R.a.msa & VC_POA_COVERAGE) {
                R.cov_of[w].resize(R.out[w].size());
                msa->coverage.insert(msa->coverage.end(), R.cov_of[w].begin(), R.cov_of[w].end());
            }
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: msa launches=%u bytes=%llu\n", R.msa_launches, (unsigned long long)msa->rows.size());
    }
    if (GraphStore* gs = R.gs) {
        auto put = [](auto& dst, const GraphPart& p, uint64_t at, uint64_t n) {
            using T = typename std::remove_reference_t<decltype(dst)>::value_type;
            const T* src = (const T*)(p.blk.data() + at);
            dst.insert(dst.end(), src, src + n);
        };
        gs->node_off.assign(1, 0); gs->aligned_off.assign(1, 0); gs->path_first.assign(1, 0); gs->path_off.assign(1, 0);
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] != VC_WIN_OK) R.part[w] = GraphPart{};
            const GraphPart& p = R.part[w];
            const GraphBlock B = graph_block(p.N, p.E, p.P, p.S, p.T, p.Cn);
            const uint64_t e0 = gs->edge_head.size(), t0 = gs->path_node.size();
            gs->n_nodes.push_back(p.N);
            if (!p.blk.empty()) {
                put(gs->node_base, p, B.base, p.N); put(gs->node_cons_pos, p, B.cons_pos, p.N); put(gs->rank_to_node, p, B.rank, p.N);
                put(gs->edge_head, p, B.head, p.E); put(gs->edge_weight, p, B.weight, p.E);
                put(gs->aligned_a, p, B.al_a, p.P); put(gs->aligned_b, p, B.al_b, p.P);
                put(gs->path_member, p, B.member, p.S); put(gs->path_reversed, p, B.rev, p.S); put(gs->path_node, p, B.p_node, p.T);
                put(gs->cons_node, p, B.cons_node, p.Cn);
                const uint32_t* oo = (const uint32_t*)(p.blk.data() + B.out_off);
                for (uint32_t v = 0; v <= p.N; ++v) gs->out_off.push_back(e0 + oo[v]);
                const uint32_t* po = (const uint32_t*)(p.blk.data() + B.p_off);
                for (uint32_t k = 1; k <= p.S; ++k) gs->path_off.push_back(t0 + po[k]);
            } else {
                gs->out_off.push_back(e0);      // a group without a block has no node and no path: its one out_off entry
            }
            gs->node_off.push_back(gs->node_base.size());
            gs->aligned_off.push_back(gs->aligned_a.size());
            gs->path_first.push_back(gs->path_member.size());
            R.part[w] = GraphPart{};
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: graph launches=%u bytes=%llu\n", R.graph_launches, (unsigned long long)gs->bytes);
    }
    if (AlignReq* A = R.al) {                                              // the queries in batch order; a group that was not computed passes its status on
        AlignStore& S = g_align;
        const bool pairs = (A->flags & VC_POA_ALIGN_PAIRS) != 0;
        if (pairs) S.pair_off.assign(A->nq + 1, 0);
        for (uint32_t w = 0; w < R.nw; ++w) {
            for (uint32_t s = A->q->win_seq_off[w]; s < A->q->win_seq_off[w + 1]; ++s) {
                if (R.status[w] != VC_WIN_OK) {
                    S.status[s] = R.status[w]; S.score[s] = 0; A->count[s] = 0;
                    if (!S.score_rev.empty()) { S.score_rev[s] = 0; S.reversed[s] = 0; }
                }
                if (!pairs) continue;
                if (A->count[s]) {
                    const std::vector<int32_t>& part = A->part[A->part_of[s]];
                    const int32_t* node = part.data() + A->first[s];
                    const int32_t* pos = node + part.size() / 2;
                    S.pair_node.insert(S.pair_node.end(), node, node + A->count[s]);
                    S.pair_pos.insert(S.pair_pos.end(), pos, pos + A->count[s]);
                }
                S.pair_off[s + 1] = S.pair_node.size();
            }
        }
        A->part.clear();
        if (R.kn.log) std::fprintf(stderr, "vc_large: align jobs=%llu launches=%llu cells=%llu bytes=%llu\n", (unsigned long long)A->jobs,
                                   (unsigned long long)A->launches, (unsigned long long)A->cells, (unsigned long long)S.bytes);
    }
    if (R.kn.log) std::fprintf(stderr, "vc_large: done alignments=%llu cells=%llu\n", (unsigned long long)R.n_align, (unsigned long long)R.n_cells);
    uint64_t o = 0;
    for (uint32_t w = 0; w < R.nw; ++w) {
        if (o + R.out[w].size() > r->cons_cap) return fail(VC_ERR_CAPACITY, "consensus buffer too small");
        if (!R.out[w].empty()) std::memcpy(r->cons + o, R.out[w].data(), R.out[w].size());
        o += R.out[w].size();
        r->cons_off[w + 1] = o;
        r->status[w] = R.status[w];
    }
    return VC_OK;
}

int run_windows(int32_t device, const LArgs& a, const vc_batch* b, std::vector<Caps>& caps, bool labels, bool spans, const Knobs& kn, vc_result* r,
                MsaStore* msa = nullptr, const vc_poa_strand_out* so = nullptr, GraphStore* gs = nullptr, AlignReq* al = nullptr) {
    const uint32_t nw = b->n_windows;
    if (hipSetDevice(device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");
    if (g_cache.device != device) { release_cache(); g_cache.device = device; }
    Run R{a, b, caps, labels, kn, msa, so, nw, b->win_seq_off[nw], b->seq_off[b->win_seq_off[nw]]};
    DevMem mem;                                                            // the batch and the strand views: held until the call ends
    if (const int rc = upload_batch(R, mem, spans)) return rc;
    if (so) if (const int rc = strand_views(R, mem)) return rc;
    if (al && al->nq) {                                                    // (a call without a query is the call without the stage)
        R.al = al;
        if (const int rc = upload_queries(R, mem)) return rc;
        g_align.status.assign(al->nq, VC_WIN_OVERFLOW); g_align.score.assign(al->nq, 0);
        if (al->flags & VC_POA_ALIGN_STRANDS) { g_align.score_rev.assign(al->nq, 0); g_align.reversed.assign(al->nq, 0); }
        al->part_of.assign(al->nq, 0); al->count.assign(al->nq, 0); al->first.assign(al->nq, 0);
    }

    // budgets from free device memory (what this library keeps cached counts as free)
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint64_t avail = free_b + g_cache.arena.bytes + g_cache.mat.bytes;
    R.arena_budget = kn.arena ? kn.arena : std::min<uint64_t>(avail / 4, 16ull << 30);
    R.mat_budget = kn.mat ? kn.mat : std::min<uint64_t>(avail / 2, 48ull << 30);
    R.gs = gs;
    if (gs) { gs->clear(); R.part.resize(nw); }
    R.planes = plane_count(a.gaps);
    R.ns = so ? 2 : 1;

    R.out.resize(nw);
    R.status.assign(nw, VC_WIN_OVERFLOW);
    if (msa) {
        R.mem_of.resize(nw); R.cov_of.resize(nw);
        msa->clear();
        msa->n_rows.assign(nw, 0); msa->row_size.assign(nw, 0); msa->row_off.assign(nw, 0); msa->member_off.assign(nw + 1, 0);
    }
    R.pending.resize(nw);
    for (uint32_t w = 0; w < nw; ++w) R.pending[w] = w;
    while (!R.pending.empty()) {
        Group G;
        next_group(R, G);
        if (G.ids.empty()) continue;
        if (const int rc = run_group(R, G)) return rc;
    }
    if (so) if (const int rc = copy_strands(R)) return rc;
    return assemble(R, r);
}

// vc_poa_run_align's own arguments, after the batch and before the device: the output and its flags, the query batch and its
// count against the groups, the query lengths
int check_queries(AlignReq& A, const vc_poa_align_out* out, const vc_batch* b) {
    if (!out) return fail(VC_ERR_ARG, "null align output");
    if (A.flags & ~(uint32_t)(VC_POA_ALIGN_PAIRS | VC_POA_ALIGN_STRANDS)) return fail(VC_ERR_ARG, "unknown align flag bits");
    const vc_batch* q = A.q;
    if (!q) return fail(VC_ERR_ARG, "null query batch");
    if (q->n_windows != b->n_windows) return fail(VC_ERR_ARG, "the query batch needs one window per group");
    const uint32_t nw = q->n_windows;
    if (nw == 0) return VC_OK;
    if (!q->win_seq_off || !q->seq_off) return fail(VC_ERR_ARG, "null array in the query batch");
    if (q->win_seq_off[0] != 0) return fail(VC_ERR_ARG, "win_seq_off[0] of the query batch must be 0");
    for (uint32_t w = 0; w < nw; ++w)
        if (q->win_seq_off[w + 1] < q->win_seq_off[w]) return fail(VC_ERR_ARG, "win_seq_off of the query batch decreases");
    const uint32_t nq = q->win_seq_off[nw];
    if (q->seq_off[0] != 0) return fail(VC_ERR_ARG, "seq_off[0] of the query batch must be 0");
    for (uint32_t s = 0; s < nq; ++s)
        if (q->seq_off[s + 1] < q->seq_off[s]) return fail(VC_ERR_ARG, "seq_off of the query batch decreases");
    if (q->seq_off[nq] && !q->bases) return fail(VC_ERR_ARG, "null bases in the query batch");
    for (uint32_t s = 0; s < nq; ++s)
        if (q->seq_off[s + 1] - q->seq_off[s] >= 65535) return fail(VC_ERR_ARG, "query length unsupported (at most 65 534 bases)");
    A.nq = nq; A.nbytes = q->seq_off[nq];
    return VC_OK;
}

// The four vc_poa_* entries after their score checks: the knobs, the batch (still without the device), the device, the run.
// `a` holds the scores.
int run_groups(int32_t device, int32_t algorithm, LArgs a, const vc_batch* b, vc_result* r, MsaStore* msa, const vc_poa_strand_out* so,
               GraphStore* gs, AlignReq* al = nullptr, const vc_poa_align_out* ao = nullptr) {
    Knobs kn;
    if (!read_knobs(kn)) return fail(VC_ERR_ARG, "VC_LARGE_CAPS: expected entries like n:4 (tables n, e, a, l, s, p; shift 0..40)");
    const uint32_t nw = b->n_windows;
    std::vector<Caps> caps(nw);
    if (nw) {
        if (!b->win_seq_off || !b->seq_off || !b->seq_has_qual) return fail(VC_ERR_ARG, "null array in batch");
        if (b->win_seq_off[0] != 0) return fail(VC_ERR_ARG, "win_seq_off[0] must be 0");
        for (uint32_t w = 0; w < nw; ++w)
            if (b->win_seq_off[w + 1] < b->win_seq_off[w]) return fail(VC_ERR_ARG, "win_seq_off decreases");
        const uint32_t nseq_all = b->win_seq_off[nw];
        if (b->seq_off[0] != 0) return fail(VC_ERR_ARG, "seq_off[0] must be 0");
        bool any_qual = false;
        for (uint32_t s = 0; s < nseq_all; ++s) {
            if (b->seq_off[s + 1] < b->seq_off[s]) return fail(VC_ERR_ARG, "seq_off decreases");
            if (b->seq_off[s + 1] - b->seq_off[s] >= 65535) return fail(VC_ERR_ARG, "sequence length unsupported (at most 65 534 bases)");
            any_qual |= b->seq_has_qual[s] != 0;
        }
        if (b->seq_off[nseq_all] && !b->bases) return fail(VC_ERR_ARG, "null bases");
        if (b->seq_off[nseq_all] && any_qual && !b->quals) return fail(VC_ERR_ARG, "null quals beside seq_has_qual");
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t s0 = b->win_seq_off[w], s1 = b->win_seq_off[w + 1];
            uint64_t mx = 0;
            for (uint32_t s = s0; s < s1; ++s) mx = std::max<uint64_t>(mx, b->seq_off[s + 1] - b->seq_off[s]);
            caps[w] = initial_caps(b->seq_off[s1] - b->seq_off[s0], mx, s1 - s0, kn);
        }
    }
    if (al) if (const int rc = check_queries(*al, ao, b)) return rc;
    if (const int rc = check_device(device)) return rc;
    r->cons_off[0] = 0;
    if (nw == 0) return VC_OK;
    a.num_prune = 1; a.mode = 2; a.algorithm = (uint32_t)algorithm;
    return run_windows(device, a, b, caps, msa != nullptr || gs != nullptr, false, kn, r, msa, so, gs, al);
}

// vc_poa_run_gaps, vc_poa_run_msa (o is required) and vc_poa_run_strand (so is required, o may be NULL); vc_poa_run after its
// own checks comes in as POA_GAPS; vc_poa_run_graph (go is required, o and so may be NULL: so chooses the strand flow).  The
// arguments first, without the device, in AlignmentEngine::Create's order (alignment_engine.cpp:39-57; spoa takes the scores as
// int8_t); then the flags, then the graph output, then the strand output; the batch in run_groups.
enum PoaCall { POA_GAPS, POA_MSA, POA_STRAND, POA_GRAPH, POA_ALIGN };

int poa_run(PoaCall call, const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* so,
            vc_poa_graph_out* go = nullptr, const vc_batch* qb = nullptr, vc_poa_align_out* ao = nullptr) {
    if (go) *go = vc_poa_graph_out{};                                      // a failed call leaves every pointer NULL
    AlignReq al;
    if (ao) { al.flags = ao->flags; *ao = vc_poa_align_out{}; ao->flags = al.flags; }
    al.q = qb;
    if (!p || !b || !r || (call == POA_MSA && !o) || !r->cons_off || !r->status || (!r->cons && r->cons_cap)) return fail(VC_ERR_ARG, "null argument");
    if (p->algorithm < 0 || p->algorithm > 2) return fail(VC_ERR_ARG, "algorithm must be 0 (local), 1 (global) or 2 (semi-global)");
    if (p->gap_open > 0 || p->gap_open2 > 0) return fail(VC_ERR_ARG, "gap opening penalties must be <= 0");
    if (p->gap_extend > 0 || p->gap_extend2 > 0) return fail(VC_ERR_ARG, "gap extension penalties must be <= 0");
    for (const int32_t s : {p->match, p->mismatch, p->gap_open, p->gap_extend, p->gap_open2, p->gap_extend2})
        if (s < -128 || s > 127) return fail(VC_ERR_ARG, "scores must lie in -128..127 (spoa's int8_t parameters)");
    const uint32_t flags = o ? o->flags : 0;
    if (flags & ~(uint32_t)(VC_POA_MSA | VC_POA_MSA_CONSENSUS | VC_POA_COVERAGE)) return fail(VC_ERR_ARG, "unknown flag bits");
    if ((flags & VC_POA_MSA_CONSENSUS) && !(flags & VC_POA_MSA)) return fail(VC_ERR_ARG, "VC_POA_MSA_CONSENSUS needs VC_POA_MSA");
    if (call == POA_GRAPH && !go) return fail(VC_ERR_ARG, "null graph output");
    if ((call == POA_STRAND && !so) || (so && !so->reversed)) return fail(VC_ERR_ARG, "null strand output (reversed is required)");
    // the subtype and its scores (alignment_engine.cpp:59-69)
    int32_t g = p->gap_open, e = p->gap_extend, q = p->gap_open2, c = p->gap_extend2;
    const uint32_t gaps = g >= e ? 0 : (g <= q || e >= c ? 1 : 2);
    if (gaps == 0) e = g;
    else if (gaps == 1) { q = g; c = e; }
    LArgs a{};
    a.match = p->match; a.mismatch = p->mismatch; a.gap = g; a.gap_e = e; a.gap_q = q; a.gap_c = c; a.gaps = gaps;
    a.msa = flags;
    a.strand = so ? 1 : 0;
    a.graph = go ? graph_route() : 0;                                      // (vc_poa_run_align may ask for the tables too)
    if (o) { *o = vc_poa_msa_out{}; o->flags = flags; }
    if (call != POA_GAPS) { g_msa.clear(); g_graph.clear(); g_align.clear(); }   // what an earlier call handed out ends here
    const int rc = run_groups(p->device, p->algorithm, a, b, r, flags ? &g_msa : nullptr, so, go ? &g_graph : nullptr,
                              call == POA_ALIGN ? &al : nullptr, ao);
    if (rc != VC_OK) {
        if (call != POA_GAPS) { g_msa.clear(); g_graph.clear(); g_align.clear(); }
        return rc;
    }
    if (call == POA_ALIGN) {
        AlignStore& S = g_align;
        ao->n_queries = al.nq;
        if (al.nq == 0) {                                                  // no stage ran: the empty tables
            S.status.clear(); S.score.clear();
            if (al.flags & VC_POA_ALIGN_PAIRS) S.pair_off.assign(1, 0);
        }
        S.status.reserve(1); S.score.reserve(1); S.score_rev.reserve(1); S.reversed.reserve(1); S.pair_node.reserve(1); S.pair_pos.reserve(1);
        ao->status = S.status.data(); ao->score = S.score.data();
        if (al.flags & VC_POA_ALIGN_STRANDS) { ao->score_rev = S.score_rev.data(); ao->reversed = S.reversed.data(); }
        if (al.flags & VC_POA_ALIGN_PAIRS) { ao->pair_off = S.pair_off.data(); ao->pair_node = S.pair_node.data(); ao->pair_pos = S.pair_pos.data(); }
        ao->bytes = S.bytes;
    }
    if (go) {
        go->n_groups = b->n_windows;
        if (b->n_windows) {
            GraphStore& G = g_graph;
            for (auto* v : {&G.n_nodes, &G.rank_to_node, &G.edge_head, &G.aligned_a, &G.aligned_b, &G.path_member, &G.path_node, &G.cons_node})
                v->reserve(1);                                             // an empty table is still a pointer
            G.node_base.reserve(1); G.path_reversed.reserve(1); G.node_cons_pos.reserve(1); G.edge_weight.reserve(1);
            go->n_nodes = G.n_nodes.data(); go->node_off = G.node_off.data(); go->node_base = G.node_base.data();
            go->node_cons_pos = G.node_cons_pos.data(); go->rank_to_node = G.rank_to_node.data();
            go->out_off = G.out_off.data(); go->edge_head = G.edge_head.data(); go->edge_weight = G.edge_weight.data();
            go->aligned_off = G.aligned_off.data(); go->aligned_a = G.aligned_a.data(); go->aligned_b = G.aligned_b.data();
            go->path_first = G.path_first.data(); go->path_member = G.path_member.data(); go->path_reversed = G.path_reversed.data();
            go->path_off = G.path_off.data(); go->path_node = G.path_node.data();
            go->cons_node = G.cons_node.data();
            go->bytes = G.bytes;
        }
    }
    if (o) o->n_groups = b->n_windows;
    if (flags && b->n_windows) {
        o->n_rows = g_msa.n_rows.data(); o->row_size = g_msa.row_size.data(); o->row_off = g_msa.row_off.data();
        o->member_off = g_msa.member_off.data(); o->row_member = g_msa.row_member.data();
        o->rows = g_msa.rows.data(); o->rows_bytes = g_msa.rows.size();
        if (flags & VC_POA_COVERAGE) o->coverage = g_msa.coverage.data();
    }
    return VC_OK;
}

}  // namespace

extern "C" {

const char* vc_large_last_error(void) { return g_err.c_str(); }

void vc_large_release(void) { release_cache(); g_msa.clear(); g_graph.clear(); g_align.clear(); }

int vc_large_run(const vc_params* p, const vc_batch* b, vc_result* r) {
    if (!p || !b || !r || !r->cons_off || !r->status || (!r->cons && r->cons_cap)) return fail(VC_ERR_ARG, "null argument");
    if (const int rc = check_device(p->device)) return rc;
    if (p->mode != 0 && p->mode != 1) return fail(VC_ERR_ARG, "mode must be 0 or 1");
    if (p->num_prune == 0) return fail(VC_ERR_ARG, "num_prune must be >= 1");
    Knobs kn;
    if (!read_knobs(kn)) return fail(VC_ERR_ARG, "VC_LARGE_CAPS: expected entries like n:4 (tables n, e, a, l, s, p; shift 0..40)");
    const uint32_t nw = b->n_windows;
    r->cons_off[0] = 0;
    if (nw == 0) return VC_OK;
    if (!b->win_seq_off || !b->seq_off || !b->seq_begin || !b->seq_end || !b->seq_has_qual || !b->bases || !b->quals || !b->win_fasta)
        return fail(VC_ERR_ARG, "null array in batch");
    // validation: what vc_submit enforces (createWindow / add_layer, window.cpp:22-27,56-67)
    std::vector<Caps> caps(nw);
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t s0 = b->win_seq_off[w], s1 = b->win_seq_off[w + 1];
        if (s1 <= s0) return fail(VC_ERR_ARG, "a window has no backbone");
        const uint64_t L = b->seq_off[s0 + 1] - b->seq_off[s0];
        if (L == 0 || L >= 65535) return fail(VC_ERR_ARG, "backbone length unsupported");
        if (!b->seq_has_qual[s0]) return fail(VC_ERR_ARG, "the backbone needs a quality string (dummy '!' for FASTA targets)");
        uint64_t sum = 0, mx = 0;
        for (uint32_t s = s0; s < s1; ++s) {
            const uint64_t len = b->seq_off[s + 1] - b->seq_off[s];
            if (len == 0 || len >= 65535) return fail(VC_ERR_ARG, "sequence length unsupported");
            if (s > s0 && (b->seq_begin[s] >= b->seq_end[s] || b->seq_begin[s] > L || b->seq_end[s] >= L)) return fail(VC_ERR_ARG, "invalid layer positions");
            sum += len; mx = std::max(mx, len);
        }
        caps[w] = initial_caps(sum, mx, s1 - s0, kn);
    }
    LArgs a{};
    a.match = p->match; a.mismatch = p->mismatch; a.gap = p->gap; a.sw_match = p->sw_match; a.sw_mismatch = p->sw_mismatch; a.sw_gap = p->sw_gap;
    a.min_conf = p->min_confidence; a.min_sup = p->min_support; a.num_prune = p->num_prune; a.mode = (uint32_t)p->mode;
    a.trim = (uint32_t)p->trim; a.window_type = (uint32_t)p->window_type;
    return run_windows(p->device, a, b, caps, p->mode == 1, true, kn, r);
}

const char* vc_poa_last_error(void) { return g_err.c_str(); }

int vc_poa_run(const vc_poa_params* p, const vc_batch* b, vc_result* r) {
    // its own struct and messages; the rest is vc_poa_run_gaps with e = q = c = g, which selects linear gaps
    if (!p || !b || !r || !r->cons_off || !r->status || (!r->cons && r->cons_cap)) return fail(VC_ERR_ARG, "null argument");
    if (p->algorithm < 0 || p->algorithm > 2) return fail(VC_ERR_ARG, "algorithm must be 0 (local), 1 (global) or 2 (semi-global)");
    if (p->gap > 0) return fail(VC_ERR_ARG, "gap must be <= 0 (linear gaps: spoa's gap opening penalty must be non-positive)");
    for (const int32_t s : {p->match, p->mismatch, p->gap})
        if (s < -128 || s > 127) return fail(VC_ERR_ARG, "scores must lie in -128..127 (spoa's int8_t parameters)");
    // poa_run repeats these checks on gp; after the ones above none of them can fire
    const vc_poa_gap_params gp{p->device, p->algorithm, p->match, p->mismatch, p->gap, p->gap, p->gap, p->gap};
    return poa_run(POA_GAPS, &gp, b, r, nullptr, nullptr);
}

int vc_poa_run_gaps(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r) { return poa_run(POA_GAPS, p, b, r, nullptr, nullptr); }

int vc_poa_run_msa(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o) { return poa_run(POA_MSA, p, b, r, o, nullptr); }

int vc_poa_run_strand(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s) {
    return poa_run(POA_STRAND, p, b, r, o, s);
}

int vc_poa_run_graph(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s,
                     vc_poa_graph_out* g) {
    return poa_run(POA_GRAPH, p, b, r, o, s, g);
}

int vc_poa_run_align(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_strand_out* s, vc_poa_graph_out* g,
                     const vc_batch* q, vc_poa_align_out* a) {
    return poa_run(POA_ALIGN, p, b, r, nullptr, s, g, q, a);
}

}  // extern "C"
