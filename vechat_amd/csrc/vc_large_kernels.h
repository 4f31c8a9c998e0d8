// The device half of the large-graph path (vc_large.hip): the tables the kernels read (LGraph, LWin, LArgs, LJob), the graph
// functions and the k_lg_* kernels, for gfx950 / wave64.  What each kernel does, the schedules and the limits: the header of
// vc_large.hip, which holds the host schedule and the C entries and is the one translation unit that includes this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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
    uint32_t gr_cols, gr_path;                         // k_lg_graph<0>: columns of the alignment (k_lg_msa<0> leaves them too for k_lg_profile), path entries (bases of the added sequences)
    // vc_poa_run_from only (0 / nullptr otherwise): the group began as a stored graph (k_lg_load).  Its first n_old sequences are
    // the stored paths -- sq_member holds their member numbers as stored, sq_len / sq_rev their lengths and strand flags --; the
    // sequences behind them are members of the batch, numbered from m0 in the outputs (seq_member, seq_len, seq_rev below)
    uint32_t n_old, m0;
    uint32_t* sq_len;                                  // [nseq]
    uint8_t* sq_rev;                                   // [nseq]
    // vc_poa_run_assign only: k_lg_slots's count of row slots of the finished graph, row 0's included; the slot of rank r is
    // map[r] (map, g2s and fr_v are free once a group has finished: k_lg_slots keeps slot, last reader and free heap in them)
    uint32_t n_slots;
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
    // mode 2, vc_poa_run_correct: 1 sends a group through the prune phases after its build (min_conf, min_sup, num_prune as in
    // mode 0; W.L / W.fasta: length of the first non-empty member, 1 where it has no quality); 0 elsewhere
    uint32_t correct;
    // mode 2, vc_poa_run_strand (strand = 1; nullptr / 0 elsewhere): the strand views of the batch, k_lg_views, laid out as bases /
    // quals are, and the choice per sequence of the batch
    uint32_t strand;
    uint32_t state;                                    // mode 2, vc_poa_run_from with a vc_poa_state_out: 1 k_lg_graph writes every node's aligned list behind its block; 0 elsewhere
    // mode 2, vc_poa_run_spans with at least one span (0 elsewhere, and seq_begin / seq_end are nullptr then): seq_begin / seq_end
    // hold, per sequence of the batch, the inclusive node range on sequence 0 of its group, or NONE / NONE for the whole graph
    uint32_t spans;
    // mode 2, vc_poa_run_weighted with at least one member of mode 1 or 2 (nullptr elsewhere, and k_lg_apply<false> runs): the mode
    // per sequence of the batch, the per-sequence weights, the per-base weights at seq_off's offsets (nullptr without a mode-2 member)
    const uint8_t* wmode;
    const uint32_t *seq_w, *base_w;
    uint32_t profile;                                  // mode 2, vc_poa_run_weighted with a vc_poa_profile_out: 1 k_lg_msa<0> runs for k_lg_profile; 0 elsewhere
    uint32_t haps;                                     // mode 2, vc_poa_run_haplotypes: 1 the edges keep their labels for k_lg_hap; 0 elsewhere
    uint8_t *rc_bases, *rv_quals, *rt_bases;           // reverse complement, reversed quality, the bytes complemented twice
    uint8_t* s_rev;                                    // [sequences] 1: the reverse complement was kept
    int32_t *s_score, *s_score_rev;                    // [sequences] both strands' scores
    uint64_t nbytes;                                   // k_lg_views: bytes of the batch
    // k_lg_fwd / k_lg_back: windows of this launch (indices into win) and their matrices (k_lg_msa<1>, k_lg_graph<1>: groups and the
    // byte offsets of their blocks in msa_out; k_lg_graph<1> has the offsets of the groups' scratch behind them, at hoff[groups + k]).
    // k_lg_load is the one other use of list: win is indexed by the block there, and list[block] is the group's index in the BATCH,
    // which is its index in the stored graphs (LLoad)
    const uint32_t* list;
    const uint64_t* hoff;
    int32_t* H;
    uint8_t* msa_out;
    // vc_poa_run_align only (nullptr elsewhere): the jobs of the query stage (k_lg_qfwd / k_lg_qback: a.list holds job indices), the
    // query batch's offsets and bytes, its reverse-complement view (VC_POA_ALIGN_STRANDS), the jobs' pair areas and the packed pairs.
    // vc_poa_run_correct's final stage fills them too: a job per member, q_off / q_bases the group batch's own arrays, algorithm 0,
    // and k_lg_correct<1> writes the corrected bytes to msa_out
    struct LJob* job;
    const uint64_t* q_off;
    const uint8_t *q_bases, *q_rc;
    int32_t *q_pairs, *q_out;
};

// One query against the finished graph of its group (vc_poa_run_align), or one member against the final pruned graph of its
// group (vc_poa_run_correct): filled by the host but for the results.
struct LJob {
    uint32_t win, qs;                                  // the group (index among the windows in flight), the query (sequence of the query batch)
    uint32_t rows, qlen, status;                       // graph rows, query length; VC_WIN_OK, or VC_WIN_INVALID from the backtrack
    uint32_t max_i[2], max_j[2];                       // end cell per strand
    int32_t score[2];                                  // spoa's *score per strand
    uint32_t rev, npairs;                              // the strand the backtrack walked, its pairs
    uint32_t ncorr;                                    // vc_poa_run_correct: the pairs with a node, k_lg_correct<0> (it takes the struct's padding)
    uint64_t area, pair_off;                           // pairs: first of the job's area (rows + qlen of them) in q_pairs, first in q_out (k_lg_correct<1>: first byte in msa_out)
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

// The weight of base i of sequence s as it is added.  WT (k_lg_apply<true>, vc_poa_run_weighted with at least one weighted member)
// puts the member's mode in front: 1 one weight for every base, 2 a weight per base at seq_off's offsets -- a kept reverse strand
// reads them back to front, as its quality --, 0 what the batch says.  Without WT the body is what it was before weights existed.
template <bool WT = false>
__device__ __forceinline__ uint32_t weight_of(const LArgs& a, const LWin& W, uint32_t s, uint32_t i, bool use_qual) {
    if constexpr (WT) {
        const uint32_t m = a.wmode[s];                                     // per lane: k_lg_apply runs one group per lane, so the lanes' modes may differ
        if (m == 1) return a.seq_w[s];
        if (m == 2) return a.base_w[a.strand && W.rev ? a.seq_off[s + 1] - 1 - i : a.seq_off[s] + i];
    }
    return use_qual ? a.lut_w[(a.strand && W.rev ? a.rv_quals : a.quals)[a.seq_off[s] + i]] : 1u;
}

// g_add_chain: fresh chain for seq[begin, end); *first = first node or NONE
template <bool WT = false>
__device__ bool add_chain(const LArgs& a, LWin& W, LGraph& g, uint32_t s, bool uq, uint32_t begin, uint32_t end, uint32_t* first) {
    *first = NONE;
    const uint8_t* seq = kept_bases(a, W, s);
    uint32_t prev = NONE;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t curr = add_node(W, g, (uint32_t)W.coder[seq[i]]);
        if (curr == NONE) return false;
        if (*first == NONE) *first = curr;
        if (prev != NONE && !add_edge(W, g, prev, curr, weight_of<WT>(a, W, s, i - 1, uq) + weight_of<WT>(a, W, s, i, uq))) return false;
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
template <bool WT = false>
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
        if (!add_chain<WT>(a, W, g, s, uq, 0, len, &first)) return -2;
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
    if (!add_chain<WT>(a, W, g, s, uq, 0, (uint32_t)vfront, &begin)) return -2;
    uint32_t prev = (begin != NONE) ? g.n_nodes - 1 : NONE;
    if (!add_chain<WT>(a, W, g, s, uq, (uint32_t)vback + 1, len, &last)) return -2;
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
        if (prev != NONE && !add_edge(W, g, prev, curr, weight_of<WT>(a, W, s, q - 1, uq) + weight_of<WT>(a, W, s, q, uq))) return -2;
        prev = curr;
    }
    if (last != NONE && !add_edge(W, g, prev, last, weight_of<WT>(a, W, s, vback, uq) + weight_of<WT>(a, W, s, vback + 1, uq))) return -2;
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

// The graph a bundle walks, its weights and its scratch.  BundleAll is the whole graph with its own weights on W's scratch, which
// is what finish_linear and finish_poa always walked; HapView (k_lg_hapcons) restricts it to one haplotype's nodes and edges.
struct BundleAll {
    const LGraph& g;
    int64_t* scores;
    uint32_t *pred, *node_rank, *comp;
    __device__ __forceinline__ bool node(uint32_t) const { return true; }
    __device__ __forceinline__ bool edge(uint32_t) const { return true; }
    __device__ __forceinline__ int64_t weight(uint32_t e) const { return g.weight[e]; }
    __device__ __forceinline__ uint32_t out_n(uint32_t v) const { return g.out_n[v]; }
};

// g_branch_completion
template <class View>
__device__ uint32_t branch_completion(const LGraph& g, const View& V, uint32_t rank) {
    int64_t* scores = V.scores;
    uint32_t* pred = V.pred;
    const uint32_t start = g.rank[rank];
    for (uint32_t o = g.out_h[start]; o != NONE; o = g.nx_out[o]) {
        if (!V.edge(o)) continue;
        const uint32_t h = g.head[o];
        for (uint32_t e = g.in_h[h]; e != NONE; e = g.nx_in[e]) {
            if (!V.edge(e)) continue;
            if (g.tail[e] != start) scores[g.tail[e]] = -1;
        }
    }
    uint32_t mx = NONE;
    for (uint32_t i = rank + 1; i < g.n_rank; ++i) {
        const uint32_t it = g.rank[i];
        if (!V.node(it)) continue;
        scores[it] = -1; pred[it] = NONE;
        for (uint32_t e = g.in_h[it]; e != NONE; e = g.nx_in[e]) {
            if (!V.edge(e)) continue;
            const uint32_t tl = g.tail[e];
            if (scores[tl] == -1) continue;
            const int64_t w = V.weight(e);
            if (scores[it] < w || (scores[it] == w && pred[it] != NONE && scores[pred[it]] <= scores[tl])) {
                scores[it] = w; pred[it] = tl;
            }
        }
        if (pred[it] != NONE) scores[it] += scores[pred[it]];
        if (mx == NONE || scores[mx] < scores[it]) mx = it;
    }
    return mx;
}

// g_heaviest_bundle -> V.comp[0 .. n) (node ids, source first)
template <class View>
__device__ uint32_t heaviest_bundle(const LGraph& g, const View& V) {
    if (g.n_rank == 0) return 0;
    const uint32_t N = g.n_nodes;
    int64_t* scores = V.scores;
    uint32_t* pred = V.pred;
    for (uint32_t i = 0; i < N; ++i) { pred[i] = NONE; scores[i] = -1; }
    uint32_t mx = NONE;
    for (uint32_t r = 0; r < g.n_rank; ++r) {
        const uint32_t it = g.rank[r];
        if (!V.node(it)) continue;
        for (uint32_t e = g.in_h[it]; e != NONE; e = g.nx_in[e]) {
            if (!V.edge(e)) continue;
            const uint32_t tl = g.tail[e];
            const int64_t w = V.weight(e);
            if (scores[it] < w || (scores[it] == w && pred[it] != NONE && scores[pred[it]] <= scores[tl])) {
                scores[it] = w; pred[it] = tl;
            }
        }
        if (pred[it] != NONE) scores[it] += scores[pred[it]];
        if (mx == NONE || scores[mx] < scores[it]) mx = it;
    }
    if (V.out_n(mx) != 0) {
        for (uint32_t r = 0; r < g.n_rank; ++r) V.node_rank[g.rank[r]] = r;
        while (V.out_n(mx) != 0) mx = branch_completion(g, V, V.node_rank[mx]);
    }
    uint32_t n = 0;
    while (pred[mx] != NONE) { V.comp[n++] = mx; mx = pred[mx]; }
    V.comp[n++] = mx;
    for (uint32_t x = 0, y = n - 1; x < y; ++x, --y) { const uint32_t t = V.comp[x]; V.comp[x] = V.comp[y]; V.comp[y] = t; }
    return n;
}
__device__ uint32_t heaviest_bundle(LWin& W, const LGraph& g) { return heaviest_bundle(g, BundleAll{g, W.scores, W.pred, W.node_rank, W.comp}); }

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

// Sequence s of a group's sequences_ as the outputs name it: its member number, its length and its strand flag.  A stored path
// (s < n_old, vc_poa_run_from) carries its own; a member of the batch is numbered from m0 and measured in the batch.
__device__ __forceinline__ uint32_t seq_member(const LWin& W, uint32_t s) { return s < W.n_old ? W.sq_member[s] : W.m0 + W.sq_member[s]; }
__device__ __forceinline__ uint32_t seq_len(const LArgs& a, const LWin& W, uint32_t s) {
    if (s < W.n_old) return W.sq_len[s];
    const uint32_t q = W.s0 + W.sq_member[s];
    return (uint32_t)(a.seq_off[q + 1] - a.seq_off[q]);
}
__device__ __forceinline__ uint8_t seq_rev(const LArgs& a, const LWin& W, uint32_t s) {
    if (s < W.n_old) return W.sq_rev[s];
    return a.strand ? a.s_rev[W.s0 + W.sq_member[s]] : 0;
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
    W.gr[0].labels = a.mode == 1 || a.msa != 0 || a.graph != 0 || a.profile != 0 || a.haps != 0; W.gr[1].labels = 0;
    W.cur = 0; W.sub = 0; W.grow = 0; W.status = 0xFF; W.rows = 0; W.npairs = 0; W.cons_n = 0; W.total = 0.0; W.avg = 0.0;
    W.msa_rows = 0; W.row_size = 0; W.rev = 0; W.gr_cols = 0; W.gr_path = 0;
    if (a.mode == 2) {                                                     // POA group: sequence 0 meets the empty graph in k_lg_prep
        W.phase = PH_BUILD; W.j = 0; W.k = 0;
        if (a.correct) {                                                   // window_len and if_fasta of window.cpp:301-309: the first non-empty member's
            W.L = 0; W.fasta = 0;
            for (uint32_t s = W.s0; s < W.s0 + W.nseq && W.L == 0; ++s) {
                W.L = (uint32_t)(a.seq_off[s + 1] - a.seq_off[s]);
                W.fasta = a.has_qual[s] == 0;
            }
        }
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

// The stored graphs of vc_poa_run_from on the device: the arrays of vc_poa_graph_in (checked by the host, check_from), and per
// group the decoder the host prepared -- the bytes in order of first appearance along the paths, which is the order in which
// add_alignment met them --, 256 bytes per group, and their count.
struct LLoad {
    const uint32_t* n_nodes;
    const uint64_t* node_off;
    const uint8_t* node_base;
    const uint32_t* rank_to_node;
    const uint64_t* out_off;
    const uint32_t* edge_head;
    const int64_t* edge_weight;
    const uint64_t* al_off;
    const uint32_t* al_node;
    const uint64_t* path_first;
    const uint32_t* path_member;
    const uint8_t* path_reversed;
    const uint64_t* path_off;
    const uint32_t* path_node;
    const uint8_t* dec;
    const uint32_t* n_codes;
};

// vc_poa_run_from: a group starts as its stored graph.  One wave per group in flight (a.list: its index in the batch), behind
// k_lg_init, which left the empty graph; the tables of W.gr[0] are filled as add_alignment would have left them, but for the ids
// of edges and cells, which nothing reads: every stage walks a node's lists in list order.
//   Nodes, lanes over nodes: the code through the coder, the rank, and the out-list and the aligned list from their CSR -- an
//     edge's id is its CSR index and its successor in the list the next index, so tail, head, weight and the links follow from
//     index arithmetic; aligned cells likewise.
//   Paths, one after the other in sequences_ order; lanes over the consecutive pairs (u, v) of path k.  A lane finds the edge in
//     u's out-list, appends label k to it (cell: the labels so far + its position in the path) and, where the edge has no label
//     yet -- this sequence created it --, appends the edge to v's in-list.  A sequence meets a node once, so within one path
//     every edge and every head is distinct and no two lanes touch the same list; successive paths are ordered by the loop and
//     its barrier.  So an edge's labels ascend, and a head's in-list holds its in-edges by first label: the order of creation.
//     Without labels only the in-lists are made (W.prank marks the edges met; graph_rows writes it anew before it is read).
// The counts are set last; a group without a new member is finished here, on its stored graph.  A table that cannot hold the
// stored graph sets W.grow like any other.
__global__ __launch_bounds__(64) void k_lg_load(LArgs a, LLoad f) {
    const uint32_t lane = threadIdx.x;
    LWin& W = a.win[blockIdx.x];
    const uint32_t w = a.list[blockIdx.x];
    LGraph& g = W.gr[0];
    const uint64_t nb = f.node_off[w], ob = nb + w, p0 = f.path_first[w];
    const uint32_t N = f.n_nodes[w], S = (uint32_t)(f.path_first[w + 1] - p0);
    const uint64_t e0 = f.out_off[ob], c0 = f.al_off[ob], t0 = f.path_off[p0];
    const uint32_t E = (uint32_t)(f.out_off[ob + N] - e0), A = (uint32_t)(f.al_off[ob + N] - c0), T = (uint32_t)(f.path_off[p0 + S] - t0);
    const bool labels = g.labels != 0;
    uint32_t grow = 0;                                                     // (the same in every lane)
    if (N > W.NC) grow |= G_NODES;
    if (E > W.EC) grow |= G_EDGES;
    if (A > W.AC) grow |= G_ALIGNED;
    if (labels && T - S > W.LC) grow |= G_LABELS;
    if (grow) { if (lane == 0) W.grow |= grow; return; }
    const uint32_t nc = f.n_codes[w];
    for (uint32_t c = lane; c < nc; c += 64) {
        const uint8_t byte = f.dec[256ull * w + c];
        W.coder[byte] = (int32_t)c; W.decoder[c] = byte;
    }
    __syncthreads();
    for (uint32_t v = lane; v < N; v += 64) {
        g.code[v] = (uint8_t)W.coder[f.node_base[nb + v]];
        g.rank[v] = f.rank_to_node[nb + v];
        g.in_h[v] = g.in_t[v] = NONE; g.in_n[v] = 0;
        const uint32_t o0 = (uint32_t)(f.out_off[ob + v] - e0), o1 = (uint32_t)(f.out_off[ob + v + 1] - e0);
        g.out_h[v] = o1 > o0 ? o0 : NONE; g.out_t[v] = o1 > o0 ? o1 - 1 : NONE; g.out_n[v] = o1 - o0;
        for (uint32_t e = o0; e < o1; ++e) {
            g.tail[e] = v; g.head[e] = f.edge_head[e0 + e]; g.weight[e] = f.edge_weight[e0 + e]; g.alive[e] = 1;
            g.nx_out[e] = e + 1 < o1 ? e + 1 : NONE; g.nx_in[e] = NONE; g.lb_h[e] = g.lb_t[e] = NONE;
            W.prank[e] = 0;
        }
        const uint32_t a0 = (uint32_t)(f.al_off[ob + v] - c0), a1 = (uint32_t)(f.al_off[ob + v + 1] - c0);
        g.al_h[v] = a1 > a0 ? a0 : NONE; g.al_t[v] = a1 > a0 ? a1 - 1 : NONE; g.al_n[v] = a1 - a0;
        for (uint32_t c = a0; c < a1; ++c) { g.al_v[c] = f.al_node[c0 + c]; g.al_nx[c] = c + 1 < a1 ? c + 1 : NONE; }
    }
    __syncthreads();
    uint32_t lb = 0;
    for (uint32_t k = 0; k < S; ++k) {
        const uint64_t po = f.path_off[p0 + k];
        const uint32_t len = (uint32_t)(f.path_off[p0 + k + 1] - po);
        const uint32_t* pn = f.path_node + po;
        if (lane == 0 && W.sq_begin) {
            W.sq_begin[k] = pn[0]; W.sq_member[k] = f.path_member[p0 + k];
            W.sq_len[k] = len; W.sq_rev[k] = f.path_reversed[p0 + k] != 0;
        }
        for (uint32_t i = lane; i + 1 < len; i += 64) {
            const uint32_t u = pn[i], v = pn[i + 1];
            uint32_t e = g.out_h[u];
            while (e != NONE && g.head[e] != v) e = g.nx_out[e];
            if (e == NONE) continue;                                       // (the host has checked that the pair is an edge)
            if (labels) {
                const uint32_t c = lb + i;
                g.lb_v[c] = k; g.lb_nx[c] = NONE;
                if (g.lb_t[e] == NONE) g.lb_h[e] = c; else g.lb_nx[g.lb_t[e]] = c;
                g.lb_t[e] = c;
            }
            if (W.prank[e] == 0) {
                W.prank[e] = 1;
                if (g.in_t[v] == NONE) g.in_h[v] = e; else g.nx_in[g.in_t[v]] = e;
                g.in_t[v] = e; g.in_n[v]++;
            }
        }
        lb += len - 1;
        __syncthreads();
    }
    if (lane == 0) {
        g.n_nodes = N; g.n_edges = E; g.n_al = A; g.n_lb = labels ? lb : 0; g.n_rank = N; g.nseq = S;
        W.num_codes = nc;
        if (W.nseq == 0) finish_poa(W);                                    // no new member: the consensus of the stored graph
    }
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
        // vc_poa_run_spans: a later member with a span meets Subgraph(begin, end) of the graph instead (window.cpp:207-213 without
        // its 1 % rule); an empty one adds nothing either way.  The host has checked the span against sequence 0, whose base k is
        // node k; a span the graph does not hold is refused here all the same, before any table is indexed with it.
        if (a.spans && W.j != 0 && a.seq_begin[W.qs] != NONE && a.seq_off[W.qs + 1] != a.seq_off[W.qs]) {
            const uint32_t sb = a.seq_begin[W.qs], se = a.seq_end[W.qs];
            if (sb > se || se >= W.gr[W.cur].n_nodes) { fail_window(W, VC_WIN_INVALID); return; }
            if (!subgraph(W, W.gr[W.cur], W.gr[1 - W.cur], sb, se)) return;
            gi = 1 - W.cur; W.sub = 1;
        }
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
    const uint32_t* slot;                              // fwd_rows<GM, true> only: rank -> row slot of the ring (k_lg_slots)
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
// SLOTS (k_lg_sfwd, vc_poa_run_assign) is the one switch: row i lives at slot W.slot[i - 1] of a ring instead of at i (row 0 at
// slot 0 either way), so the planes hold n_slots rows and only the score of the end cell means anything afterwards.  A row
// shares its slot with no row it reads and with no row a later row still reads (k_lg_slots), so the cells computed, the order of
// the maxima and the barrier per row are the same.
template <uint32_t GM, bool SLOTS = false>
__device__ __forceinline__ EndCell fwd_rows(const AlnView& W, const Mat& M) {
    const uint32_t lane = threadIdx.x;
    const uint32_t N = W.rows, len = W.len;
    const uint64_t w = M.w;
    int32_t *const H = M.H, *const F = M.F, *const E = M.E, *const O = M.O, *const Q = M.Q;
    const bool sw = W.type == 0, ov = W.type == 2;
    const int32_t m = W.m, x = W.x, gp = W.g, ge = GM == 0 ? gp : W.e, gq = W.q, gc = W.c;
    const uint8_t* seq = W.seq;
    auto row_at = [&](uint64_t i) -> uint64_t {                        // where row i begins in a plane
        if constexpr (SLOTS) return (i ? (uint64_t)W.slot[i - 1] : 0) * w;
        else return i * w;
    };
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
        const uint64_t i = (uint64_t)r + 1, ro = row_at(i);
        const uint32_t po = W.poff[r], pe = W.poff[r + 1];
        const uint8_t ch = W.rchar[r];
        const bool sink = W.sink[r] != 0;
        const int32_t* F0 = GM == 0 ? H : F;                           // column 0's vertical chain
        int32_t f0 = pe == po ? gp - ge : KNEG, o0 = pe == po ? gq - gc : KNEG;
        for (uint32_t k = po; k < pe; ++k) {
            f0 = max(f0, F0[row_at(W.prank[k])]);
            if constexpr (GM == 2) o0 = max(o0, O[row_at(W.prank[k])]);
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
                uint64_t p = pe == po ? 0 : row_at(W.prank[po]);
                int32_t d = H[p + j - 1] + s, f = vertical(p + j), o = KNEG;
                if constexpr (GM == 2) o = max(H[p + j] + gq, O[p + j] + gc);
                for (uint32_t k = po + 1; k < pe; ++k) {
                    p = row_at(W.prank[k]);
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

// ------------------------------------------------------------------ vc_poa_run_assign: every query against every group, scores only
// The slots of a finished graph's rows, one lane per group behind k_lg_rows.  Row i (rank i - 1) is read by its successors only,
// so it is dead once the last of them is complete: last[r] is the highest row that reads row r + 1 (the row itself where nobody
// does), found from poff / prank in one pass because the ranks ascend.  Then the rows upward with a free list: a row takes the
// LOWEST free slot (a binary min-heap; a fresh slot when none is free), and only when it is complete do the rows it read last --
// and the row itself, when nobody reads it -- give their slots back.  So a row shares a slot neither with a row it reads nor with
// one that a later row still reads.  Row 0, which every source reads, keeps slot 0 for good.  Deterministic: the same rule in
// Python (tests/poa_assign_ref.py) gives the same slots.
__global__ __launch_bounds__(64) void k_lg_slots(LArgs a) {
    const uint32_t w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.n) return;
    LWin& W = a.win[w];
    W.n_slots = 0;
    if (W.phase != PH_DONE || W.grow || W.status != VC_WIN_OK) return;
    const uint32_t N = W.gr[W.cur].n_nodes;
    if (W.gr[W.cur].n_rank != N) return;                                   // (the host makes no job for such a graph)
    uint32_t *const slot = W.map, *const last = W.g2s, *const heap = W.fr_v;
    for (uint32_t r = 0; r < N; ++r) last[r] = r + 1;
    for (uint32_t r = 0; r < N; ++r)
        for (uint32_t k = W.poff[r]; k < W.poff[r + 1]; ++k) if (W.prank[k]) last[W.prank[k] - 1] = r + 1;
    uint32_t nh = 0, ns = 1;
    auto give = [&](uint32_t s) {
        uint32_t c = nh++;
        for (; c && heap[(c - 1) / 2] > s; c = (c - 1) / 2) heap[c] = heap[(c - 1) / 2];
        heap[c] = s;
    };
    auto take = [&]() -> uint32_t {
        if (!nh) return ns++;
        const uint32_t s = heap[0], x = heap[--nh];
        uint32_t c = 0;
        for (;;) {
            uint32_t k = 2 * c + 1;
            if (k >= nh) break;
            if (k + 1 < nh && heap[k + 1] < heap[k]) ++k;
            if (heap[k] >= x) break;
            heap[c] = heap[k]; c = k;
        }
        if (nh) heap[c] = x;
        return s;
    };
    for (uint32_t r = 0; r < N; ++r) {
        const uint32_t s = take();
        slot[r] = s;
        for (uint32_t k = W.poff[r]; k < W.poff[r + 1]; ++k) {
            const uint32_t p = W.prank[k];
            if (p && last[p - 1] == r + 1) { give(slot[p - 1]); last[p - 1] = NONE; }   // (NONE: an edge listed twice gives once)
        }
        if (last[r] == r + 1) give(s);
    }
    W.n_slots = ns;
}

// One (query, group) pair of vc_poa_run_assign: fwd_rows on the ring of the group's slots, n_slots x (len + 1) cells per plane
// in place of (rows + 1) x (len + 1), on a grid of (pairs of the launch, strands).  It leaves the score in the job, nothing else.
template <uint32_t GM>
__global__ __launch_bounds__(64) void k_lg_sfwd(LArgs a) {
    LJob& J = a.job[a.list[blockIdx.x]];
    const uint32_t st = blockIdx.y;
    const LWin& W = a.win[J.win];
    AlnView V = query_view(a, W, J, st);
    V.slot = W.map;
    const EndCell b = fwd_rows<GM, true>(V, matrix_of<GM>(a, blockIdx.x, W.n_slots - 1, J.qlen, st));
    if (threadIdx.x == 0) J.score[st] = b.s;
}

// What k_lg_assign folds into, per query of the call (device arrays that live as long as the call), and the chunk of pairs at
// hand: the pairs of a batch of resident groups are numbered query-major over its `nfin` finished groups, pair t being query
// t / nfin against the (t % nfin)-th of them, and a.job holds the pairs t0 .. t1 - 1.
struct LAssign {
    const uint32_t* gid;                               // [windows in flight] the group's index in the call
    uint64_t t0, t1;
    uint32_t nfin, ng, strands;
    int32_t *best_g, *best_s, *sec_g, *sec_s;          // [queries]
    uint8_t *rev, *flag;                               // [queries] the strand kept against best_g; 1: a pair overflowed, 2: a pair was invalid
    int32_t* scores;                                   // [queries x ng], nullptr without VC_POA_ASSIGN_SCORES
    uint8_t* pair_status;
};

// One lane per query with a pair in the chunk: its pairs, which lie side by side in group order, folded into the running best
// and second.  A pair is ranked when it is VC_WIN_OK and its group has a node; it replaces on a greater score, or on an equal
// one from a lower group, so neither the chunks nor the order in which groups became resident show in the result.  No atomics:
// a query has one lane per launch, and the launches of a call follow one another.
__global__ __launch_bounds__(64) void k_lg_assign(LArgs a, LAssign s) {
    const uint64_t k = s.t0 / s.nfin + (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (k > (s.t1 - 1) / s.nfin) return;
    const uint64_t lo = max(s.t0, k * s.nfin), hi = min(s.t1, (k + 1) * s.nfin);
    int32_t bg = s.best_g[k], bs = s.best_s[k], cg = s.sec_g[k], cs = s.sec_s[k];
    uint8_t brev = s.rev[k], fl = s.flag[k];
    for (uint64_t t = lo; t < hi; ++t) {
        const LJob& J = a.job[t - s.t0];
        const LWin& W = a.win[J.win];
        const int32_t g = (int32_t)s.gid[J.win];
        const bool ok = J.status == VC_WIN_OK, rv = ok && s.strands == 2 && J.score[0] < J.score[1];
        const int32_t sc = ok ? J.score[rv ? 1 : 0] : 0;
        if (J.status == VC_WIN_OVERFLOW) fl |= 1;
        else if (!ok) fl |= 2;
        if (s.scores) { s.scores[k * s.ng + g] = sc; s.pair_status[k * s.ng + g] = (uint8_t)J.status; }
        if (!ok || W.gr[W.cur].n_nodes == 0) continue;
        if (bg < 0 || sc > bs || (sc == bs && g < bg)) { cg = bg; cs = bs; bg = g; bs = sc; brev = rv; }
        else if (cg < 0 || sc > cs || (sc == cs && g < cg)) { cg = g; cs = sc; }
    }
    s.best_g[k] = bg; s.best_s[k] = bs; s.sec_g[k] = cg; s.sec_s[k] = cs; s.rev[k] = brev; s.flag[k] = fl;
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

// GenerateCorrectedSequence (graph.cpp:1167-1179) of every member of vc_poa_run_correct, one wave per job: of the job's pairs
// (k_lg_qback, against the final pruned graph of its group) those with a node are kept, as the decoded byte of the node.
//   PH 0: J.ncorr, the kept pairs, for the host's prefix offsets.
//   PH 1: the bytes, compact at a.msa_out + J.pair_off: per tile of 64 pairs a 64-bit ballot of `keep`, the lane's slot from the
//     population count of the lower lanes plus the total carried over the tiles before.  A store lies below J.ncorr, the job's own
//     extent, and a node below the graph's count.
template <uint32_t PH>
__global__ __launch_bounds__(64) void k_lg_correct(LArgs a) {
    LJob& J = a.job[blockIdx.x];
    const uint32_t lane = threadIdx.x, np = J.npairs;
    if (np == 0) { if (PH == 0 && lane == 0) J.ncorr = 0; return; }        // (no forward pass, an empty alignment or a refused job: no area to read)
    const int2* src = (const int2*)(a.q_pairs + 2 * J.area);
    const LWin& W = a.win[J.win];
    const LGraph& g = W.gr[W.cur];
    uint8_t* out = a.msa_out + J.pair_off;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < np; base += 64) {
        const uint32_t k = base + lane;
        const int32_t node = k < np ? src[k].x : -1;
        const bool keep = node != -1;
        const uint64_t b = __ballot(keep);
        if constexpr (PH == 1) {
            const uint32_t slot = carry + (uint32_t)__popcll(b & ((1ull << lane) - 1));
            if (keep && slot < J.ncorr && (uint32_t)node < g.n_nodes) out[slot] = (uint8_t)W.decoder[g.code[node]];
        }
        carry += (uint32_t)__popcll(b);
    }
    if (PH == 0 && lane == 0) J.ncorr = carry;
}

// WT: the call has a weighted member (LArgs::wmode is set); the plain instance is the kernel as it was
template <bool WT>
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
        const int rc = add_alignment<WT>(a, W, W.gr[W.cur], W.pairs, np, s, hq);
        if (rc == -2) return;
        if (rc) { fail_window(W, VC_WIN_INVALID); return; }
        if (a.strand) { a.s_rev[s] = (uint8_t)W.rev; a.s_score[s] = W.score[0]; a.s_score_rev[s] = W.score[1]; }
        if (a.mode == 0 || a.correct) {
            const uint32_t len = (uint32_t)(a.seq_off[s + 1] - a.seq_off[s]);
            if (!hq) W.total += (double)len;
            else for (uint32_t q = 0; q < len; ++q) W.total += a.lut_d[a.quals[a.seq_off[s] + q]];
        }
        if (++W.j < W.nseq) return;
        if (a.mode == 1) { finish_linear(a, W); return; }
        if (a.mode == 2) {
            finish_poa(W);                                                 // the consensus of the unpruned graph, whatever follows
            if (!a.correct || W.L == 0) return;                            // (L == 0: no non-empty member, nothing to prune or correct)
            W.avg = W.fasta ? 2.0 * W.total / W.L : 2.0 * W.total / W.L * 1000;
            if (!prune_and_keep_largest(a, W)) return;                     // (a table filled: the group runs again)
            W.j = 0; W.k = 0;
            if (a.num_prune > 1) W.phase = PH_ROUND;                       // else done: the correction stage reads W.gr[W.cur]
            return;
        }
        const uint16_t window_len = (uint16_t)W.L;                         // window.cpp:216
        W.avg = W.fasta ? 2.0 * W.total / window_len : 2.0 * W.total / window_len * 1000;
        if (!prune_and_keep_largest(a, W)) return;
        W.j = 0; W.k = 0;
        W.phase = a.num_prune > 1 ? PH_ROUND : PH_FINAL;
    } else if (W.phase == PH_ROUND) {
        // the backbone's qualities_[0].first is never nullptr: quality overload (a dummy '!' gives 0); a group has no backbone
        if (!add_weights(a, W, W.gr[W.cur], W.pairs, np, s, a.mode != 2 && W.j == 0 ? true : hq)) return;
        if (++W.j < W.nseq) return;
        if (!prune_and_keep_largest(a, W)) return;
        W.j = 0;
        if (++W.k + 1 >= a.num_prune) W.phase = a.mode == 2 ? PH_DONE : PH_FINAL;      // a group's members are corrected side by side, k_lg_correct
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
        if (!(a.msa & VC_POA_MSA) && !a.profile) return;
        const uint32_t cols = msa_columns(W, g, lane);
        if (lane == 0 && (a.msa & VC_POA_MSA)) { W.row_size = cols; W.msa_rows = g.nseq + ((a.msa & VC_POA_MSA_CONSENSUS) ? 1u : 0u); }
        if (lane == 0 && a.profile) W.gr_cols = cols;                      // (k_lg_graph<0> writes the same number)
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
        for (uint32_t s = lane; s < W.msa_rows; s += 64) mem[s] = s < g.nseq ? seq_member(W, s) : VC_POA_ROW_CONSENSUS;
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

// A finished group's block of k_lg_profile: (codes + 1) rows of cons_n uint32 (the last row the gaps), then the group's decoder,
// a byte per code; beside it the stage's scratch: the consensus position of every column (NONE: none), then first and last hit
// position per added sequence.  Every part is 16-byte aligned and padded to 16 bytes (the fills store whole uint4).
struct ProfileBlock { uint64_t codes, bytes; };
__host__ __device__ inline ProfileBlock profile_block(uint64_t nc, uint64_t Cn) {
    ProfileBlock B;
    B.codes = (4 * (nc + 1) * Cn + 15) & ~15ull;
    B.bytes = B.codes + ((nc + 15) & ~15ull);
    return B;
}
struct ProfileScratch { uint64_t first, last, bytes; };
__host__ __device__ inline ProfileScratch profile_scratch(uint64_t S, uint64_t cols) {
    ProfileScratch X;
    X.first = (4 * cols + 15) & ~15ull;
    X.last = X.first + ((4 * S + 15) & ~15ull);
    X.bytes = X.last + ((4 * S + 15) & ~15ull);
    return X;
}

// The verbose summary of GenerateConsensus(&summary, true), graph.cpp:486-529, of a finished POA group whose columns k_lg_msa<0>
// has left in W.map / W.gr_cols: one wave per group of a.list, block at a.msa_out + a.hoff[block], scratch at hoff[groups + block].
// The reference walks every sequence with Successor(i) and a cursor c into the consensus: a node whose column is the column of
// consensus position c counts its code there, and the positions strictly between two consecutive hits of one sequence count a
// gap.  Columns rise strictly along a sequence's path and along the consensus, so a sequence meets a consensus column at most
// once and its hits come in rising position: the hits are a scatter over the begin nodes and the label cells (the nodes of
// sequence i are its begin node and the head of every edge with label i, as in k_lg_msa<1>), and the gaps of position j are the
// sequences with first hit <= j <= last hit less the hits at j.  The first term is a difference array over the gap row -- +1 at a
// sequence's first hit, -1 behind its last -- and a wave prefix sum in tiles of 64 with a carried total; uint32 wraps as int32 does.
__global__ __launch_bounds__(64) void k_lg_profile(LArgs a) {
    const uint32_t lane = threadIdx.x;
    LWin& W = a.win[a.list[blockIdx.x]];
    const LGraph& g = W.gr[W.cur];
    const uint32_t nc = W.num_codes, Cn = W.cons_n, S = g.nseq;
    const ProfileBlock B = profile_block(nc, Cn);
    const ProfileScratch X = profile_scratch(S, W.gr_cols);
    uint8_t* blk = a.msa_out + a.hoff[blockIdx.x];                         // both 16-byte aligned
    uint8_t* scr = a.msa_out + a.hoff[gridDim.x + blockIdx.x];
    uint32_t* counts = (uint32_t*)blk;
    uint32_t *cpos = (uint32_t*)scr, *first = (uint32_t*)(scr + X.first), *last = (uint32_t*)(scr + X.last);
    uint4 *b4 = (uint4*)blk, *s4 = (uint4*)scr;
    for (uint64_t k = lane; k < B.bytes / 16; k += 64) b4[k] = make_uint4(0, 0, 0, 0);
    for (uint64_t k = lane; k < X.last / 16; k += 64) s4[k] = make_uint4(NONE, NONE, NONE, NONE);
    for (uint64_t k = X.last / 16 + lane; k < X.bytes / 16; k += 64) s4[k] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (uint32_t k = lane; k < nc; k += 64) blk[B.codes + k] = (uint8_t)W.decoder[k];
    for (uint32_t i = lane; i < Cn; i += 64) cpos[W.map[W.comp[i]]] = i;
    __syncthreads();
    for (uint32_t s = lane; s < S; s += 64) {
        const uint32_t v = W.sq_begin[s], p = cpos[W.map[v]];
        if (p == NONE) continue;
        atomicAdd(&counts[(uint64_t)g.code[v] * Cn + p], 1u);
        atomicMin(&first[s], p); atomicMax(&last[s], p);
    }
    for (uint32_t e = lane; e < g.n_edges; e += 64) {
        const uint32_t h = g.head[e], p = cpos[W.map[h]];
        if (p == NONE) continue;
        uint32_t* row = counts + (uint64_t)g.code[h] * Cn;
        for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) {
            const uint32_t s = g.lb_v[c];
            atomicAdd(&row[p], 1u);
            atomicMin(&first[s], p); atomicMax(&last[s], p);
        }
    }
    __syncthreads();
    uint32_t* gaps = counts + (uint64_t)nc * Cn;
    for (uint32_t s = lane; s < S; s += 64) {
        if (first[s] == NONE) continue;                                    // the sequence touches no consensus column
        atomicAdd(&gaps[first[s]], 1u);
        if (last[s] + 1 < Cn) atomicAdd(&gaps[last[s] + 1], NONE);         // -1
    }
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < Cn; base += 64) {
        const uint32_t j = base + lane;
        const uint32_t x = wave_scan(j < Cn ? gaps[j] : 0u, lane);
        if (j < Cn) {
            uint32_t hits = 0;
            for (uint32_t k = 0; k < nc; ++k) hits += counts[(uint64_t)k * Cn + j];
            gaps[j] = carry + x - hits;
        }
        carry += __shfl(x, 63, 64);
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
// The state table of vc_poa_state_out, behind the block when LArgs::state asks for it: N + 1 offsets into A aligned-list cells,
// then the cells, each part padded to 16 bytes.
__host__ __device__ inline uint64_t state_list_at(uint64_t N) { return (4 * (N + 1) + 15) & ~15ull; }
__host__ __device__ inline uint64_t state_bytes(uint64_t N, uint64_t A) { return state_list_at(N) + ((4 * A + 15) & ~15ull); }
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
//     while printing).  With LArgs::state (vc_poa_state_out) every node's whole aligned list follows behind the block, in list
//     order: offsets from a wave prefix sum of al_n, as out_off is made, then every lane walks its own node's list.
template <uint32_t PH>
__global__ __launch_bounds__(64) void k_lg_graph(LArgs a) {
    const uint32_t lane = threadIdx.x;
    if constexpr (PH == 0) {
        LWin& W = a.win[blockIdx.x];
        if (W.phase != PH_DONE || W.grow || W.status != VC_WIN_OK) return;
        const LGraph& g = W.gr[W.cur];
        const uint32_t cols = msa_columns(W, g, lane);
        uint32_t t = 0;
        for (uint32_t s = lane; s < g.nseq; s += 64) t += seq_len(a, W, s);
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
        const uint32_t A = a.state ? g.n_al : 0;                           // the state table behind the block: al_off, al_node
        uint32_t *st_off = (uint32_t*)(out + B.bytes), *st_node = (uint32_t*)(out + B.bytes + state_list_at(N));
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
                len = seq_len(a, W, s);
                member[s] = seq_member(W, s);
                rev[s] = seq_rev(a, W, s);
            }
            const uint32_t x = wave_scan(len, lane);
            if (s < S) p_off[s] = carry + x - len;
            carry += __shfl(x, 63, 64);
        }
        if (lane == 0) p_off[S] = carry;
        __syncthreads();
        for (uint32_t i = lane; i < Cn; i += 64) { cons_pos[W.comp[i]] = (int32_t)i; cons_node[i] = W.comp[i]; }
        // out-edges and aligned pairs
        uint32_t ce = 0, cp = 0, ca = 0;
        for (uint32_t v0 = 0; v0 < N; v0 += 64) {
            const uint32_t v = v0 + lane;
            uint32_t ne = 0, np = 0, na = 0;
            if (v < N) {
                ne = g.out_n[v];
                for (uint32_t q = g.al_h[v]; q != NONE; q = g.al_nx[q]) np += g.al_v[q] > v;
                na = g.al_n[v];
            }
            const uint32_t xe = wave_scan(ne, lane), xp = wave_scan(np, lane);
            if (a.state) {                                                 // every node's whole aligned list, in list order
                const uint32_t xa = wave_scan(na, lane);
                if (v < N) {
                    uint32_t k = ca + xa - na;
                    st_off[v] = k;
                    for (uint32_t q = g.al_h[v]; q != NONE && k < A; q = g.al_nx[q], ++k) st_node[k] = g.al_v[q];
                }
                ca += __shfl(xa, 63, 64);
            }
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
        if (a.state && lane == 0) st_off[N] = ca;
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

// ------------------------------------------------------------------ haplotypes (vc_poa_run_haplotypes; the rule: vechat_hip.h)
// What the call's kernels read beside LArgs: the rule's parameters.
struct LHap { uint32_t max_haps, min_reads, min_permille, rounds, flags; };

// A finished group's block of k_lg_hap / k_lg_hapcons, the byte offset of every table in it (16-byte aligned and padded): the
// header -- n_haps, sites, then per haplotype its members and its consensus length --, the haplotype and the group member of every
// added sequence, the sites (at most one per column), and room for max_haps consensus paths of at most N nodes.
struct HapBlock { uint64_t hap_of, member, s_col, s_n1, s_n2, s_maj, s_min, cons, bytes; };
constexpr uint32_t kHapHead = 2 + 2 * VC_POA_HAP_MAX;  // uint32 entries of the header
__host__ __device__ inline HapBlock hap_block(uint64_t S, uint64_t C, uint64_t N, uint64_t maxh) {
    HapBlock B;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = off; off += (bytes + 15) & ~15ull; return at; };
    take(4 * kHapHead);
    B.hap_of = take(S); B.member = take(4 * S);
    B.s_col = take(4 * C); B.s_n1 = take(4 * C); B.s_n2 = take(4 * C); B.s_maj = take(C); B.s_min = take(C);
    B.cons = take(maxh * N);
    B.bytes = off;
    return B;
}
// ... and its scratch, which never leaves the device: the S x C matrix of node ids, first and last column, path offsets and the
// compact paths (T entries), the two alleles of every site, the S x M votes (M <= C), every member's count of non-zero votes
// and its d(s), the profiles, and per haplotype the restricted graph of k_lg_hapcons with the bundle's scratch.  The votes live
// here, in HBM behind the L2, not in LDS: S x M has no bound that LDS could promise, and every pass over them is a stream.
struct HapScratch { uint64_t first, last, p_off, p_node, a1, a2, votes, nz, d, prof, per_hap, hap_bytes, h_wt, h_scores, h_pred, h_comp, h_outn, h_nrank, h_eset, h_nset, bytes; };
__host__ __device__ inline HapScratch hap_scratch(uint64_t S, uint64_t C, uint64_t T, uint64_t N, uint64_t E, uint64_t maxh) {
    HapScratch X;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t at = off; off += (bytes + 15) & ~15ull; return at; };
    take(4 * S * C);
    X.first = take(4 * S); X.last = take(4 * S); X.p_off = take(4 * (S + 1)); X.p_node = take(4 * T);
    X.a1 = take(4 * C); X.a2 = take(4 * C); X.votes = take(S * C); X.nz = take(4 * S); X.d = take(4 * S); X.prof = take(maxh * C);
    X.per_hap = off;
    off = 0;
    X.h_wt = take(8 * E); X.h_scores = take(8 * N); X.h_pred = take(4 * N); X.h_comp = take(4 * N); X.h_outn = take(4 * N);
    X.h_nrank = take(4 * N); X.h_eset = take(E); X.h_nset = take(N);
    X.hap_bytes = off;
    X.bytes = X.per_hap + maxh * X.hap_bytes;
    return X;
}

// the lane-wise best of (value, index) over the wave, smaller value first and then the smaller index; every lane gets it
__device__ __forceinline__ void wave_argmin(int32_t& v, uint32_t& i) {
    for (uint32_t d = 32; d; d >>= 1) {
        const int32_t ov = __shfl_xor(v, d, 64);
        const uint32_t oi = __shfl_xor(i, d, 64);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// agree(x, y) of two vote (or profile) rows of M int8
__device__ __forceinline__ int32_t hap_agree(const int8_t* x, const int8_t* y, uint32_t M) {
    int32_t t = 0;
    for (uint32_t m = 0; m < M; ++m) t += (int32_t)x[m] * (int32_t)y[m];
    return t;
}

// The members of a finished POA group split into haplotypes, one wave per group (rules 1 to 7 of vechat_hip.h).
// There is no sizing kernel of this stage's own: the sizing phase is k_lg_graph<0>, which leaves the columns in W.map /
// W.gr_cols and the path entries in W.gr_path; the host sizes block and scratch from these two and from the group's sequences,
// nodes and edges (hap_block, hap_scratch).  Then, for the groups of a.list, block at a.msa_out + a.hoff[block], scratch at
// a.hoff[groups + block]: the nodes scattered into the S x C matrix as the path stage of
// k_lg_graph<1> does; every row compacted into its path, which also finds first and last; counts with a lane per column (a row's
// loads are coalesced), one allele at a time so that only the best two live in registers; sites compacted by a wave prefix sum
// in tiles of 64 with a carried total; the votes; seeds with a lane per member and a wave arg-min that carries the label for the
// tie; rounds with a lane per member for the assignment and a lane per site for the profiles; small clusters; the order.
__global__ __launch_bounds__(64) void k_lg_hap(LArgs a, LHap hp) {
    const uint32_t lane = threadIdx.x;
    __shared__ uint32_t sh_size[VC_POA_HAP_MAX], sh_min[VC_POA_HAP_MAX], sh_map[VC_POA_HAP_MAX], sh_seed[VC_POA_HAP_MAX];
    __shared__ uint32_t sh_k;
    LWin& W = a.win[a.list[blockIdx.x]];
    const LGraph& g = W.gr[W.cur];
    const uint32_t S = g.nseq, C = W.gr_cols, T = W.gr_path, N = g.n_nodes, E = g.n_edges, nc = W.num_codes;
    const uint32_t GAP = nc, maxh = hp.max_haps;
    const HapBlock B = hap_block(S, C, N, maxh);
    const HapScratch X = hap_scratch(S, C, T, N, E, maxh);
    uint8_t* out = a.msa_out + a.hoff[blockIdx.x];
    uint8_t* scr = a.msa_out + a.hoff[gridDim.x + blockIdx.x];
    uint32_t* head = (uint32_t*)out;
    uint8_t* hap_of = out + B.hap_of;
    uint32_t *member = (uint32_t*)(out + B.member), *s_col = (uint32_t*)(out + B.s_col), *s_n1 = (uint32_t*)(out + B.s_n1), *s_n2 = (uint32_t*)(out + B.s_n2);
    uint8_t *s_maj = out + B.s_maj, *s_min = out + B.s_min;
    uint32_t *mat = (uint32_t*)scr, *first = (uint32_t*)(scr + X.first), *last = (uint32_t*)(scr + X.last), *p_off = (uint32_t*)(scr + X.p_off);
    uint32_t *p_node = (uint32_t*)(scr + X.p_node), *a1 = (uint32_t*)(scr + X.a1), *a2 = (uint32_t*)(scr + X.a2), *nz = (uint32_t*)(scr + X.nz);
    int32_t* dd = (int32_t*)(scr + X.d);
    int8_t *votes = (int8_t*)(scr + X.votes), *prof = (int8_t*)(scr + X.prof);
    if (lane < kHapHead) head[lane] = 0;
    if (S == 0) {                                                      // no non-empty member: one haplotype without a member
        if (lane == 0) head[0] = 1;
        return;
    }
    const uint64_t cells = (uint64_t)S * C;
    const uint4 none4 = make_uint4(NONE, NONE, NONE, NONE);
    for (uint64_t k = lane; k < (cells + 3) / 4; k += 64) ((uint4*)mat)[k] = none4;
    uint32_t carry = 0;
    for (uint32_t s0 = 0; s0 < S; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t len = 0;
        if (s < S) { len = seq_len(a, W, s); member[s] = seq_member(W, s); }
        const uint32_t x = wave_scan(len, lane);
        if (s < S) p_off[s] = carry + x - len;
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) p_off[S] = carry;
    __syncthreads();
    for (uint32_t s = lane; s < S; s += 64) {
        const uint32_t v = W.sq_begin[s];
        mat[(uint64_t)s * C + W.map[v]] = v;
    }
    for (uint32_t e = lane; e < E; e += 64) {
        const uint32_t h = g.head[e];
        const uint64_t col = W.map[h];
        for (uint32_t c = g.lb_h[e]; c != NONE; c = g.lb_nx[c]) mat[(uint64_t)g.lb_v[c] * C + col] = h;
    }
    __syncthreads();
    // the paths, and with them first and last
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t* row = mat + (uint64_t)s * C;
        const uint32_t end = p_off[s + 1];
        uint32_t at = p_off[s];
        for (uint32_t c0 = 0; c0 < C; c0 += 64) {
            const uint32_t c = c0 + lane;
            const uint32_t v = c < C ? row[c] : NONE;
            const uint32_t x = wave_scan(v != NONE, lane);
            const uint32_t tot = __shfl(x, 63, 64);
            if (v != NONE) {
                const uint32_t k = at + x - 1;
                if (k < end) p_node[k] = v;
                if (k == p_off[s]) first[s] = c;
                if (x == tot) last[s] = c;                             // (a later tile with a node overwrites it)
            }
            at += tot;
        }
    }
    __syncthreads();
    // counts and sites
    const bool indels = (hp.flags & VC_POA_HAP_INDELS) != 0;
    const uint32_t n_alleles = nc + (indels ? 1u : 0u);
    uint32_t M = 0;
    for (uint32_t c0 = 0; c0 < C; c0 += 64) {
        const uint32_t c = c0 + lane;
        uint32_t b1 = NONE, b2 = NONE, n1 = 0, n2 = 0;
        if (c < C) {
            uint32_t span = 0;
            for (uint32_t s = 0; s < S; ++s) span += first[s] <= c && c <= last[s];
            for (uint32_t al = 0; al < n_alleles; ++al) {
                uint32_t n = 0;
                for (uint32_t s = 0; s < S; ++s) {
                    const uint32_t v = mat[(uint64_t)s * C + c];
                    n += v != NONE ? g.code[v] == al : (al == GAP && first[s] < c && c < last[s]);
                }
                if (n < hp.min_reads || 1000ull * n < (uint64_t)hp.min_permille * span) continue;
                if (n > n1) { b2 = b1; n2 = n1; b1 = al; n1 = n; }
                else if (n > n2) { b2 = al; n2 = n; }
            }
        }
        const uint32_t site = b2 != NONE;
        const uint32_t x = wave_scan(site, lane);
        if (site) {
            const uint32_t m = M + x - 1;
            s_col[m] = c; s_n1[m] = n1; s_n2[m] = n2; a1[m] = b1; a2[m] = b2;
            s_maj[m] = b1 == GAP ? (uint8_t)'-' : (uint8_t)W.decoder[b1];
            s_min[m] = b2 == GAP ? (uint8_t)'-' : (uint8_t)W.decoder[b2];
        }
        M += __shfl(x, 63, 64);
    }
    __syncthreads();
    // votes, and every member's count of non-zero ones
    for (uint32_t s = 0; s < S; ++s) {
        uint32_t cnt = 0;
        for (uint32_t m = lane; m < M; m += 64) {
            const uint32_t c = s_col[m], v = mat[(uint64_t)s * C + c];
            const uint32_t sym = v != NONE ? g.code[v] : (first[s] < c && c < last[s] ? GAP : NONE);
            const int8_t vote = sym == a1[m] ? 1 : sym == a2[m] ? -1 : 0;
            votes[(uint64_t)s * M + m] = vote;
            cnt += vote != 0;
        }
        for (uint32_t d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) nz[s] = cnt;
    }
    __syncthreads();
    // seeds
    int32_t bv = INT32_MAX;
    uint32_t bi = NONE;
    for (uint32_t s = lane; s < S; s += 64) {
        const int32_t v = -(int32_t)nz[s];
        if (v < bv) { bv = v; bi = s; }                                // (a lane's own members come in rising label)
        dd[s] = INT32_MIN;
    }
    wave_argmin(bv, bi);
    uint32_t K = 1;
    if (lane == 0) sh_seed[0] = bi;
    __syncthreads();
    if (bv != 0) {
        for (; K < maxh; ++K) {
            const int8_t* sv = votes + (uint64_t)sh_seed[K - 1] * M;
            int32_t mv = INT32_MAX;
            uint32_t mi = NONE;
            for (uint32_t s = lane; s < S; s += 64) {
                const int32_t ag = hap_agree(votes + (uint64_t)s * M, sv, M);
                const int32_t d = dd[s] > ag ? dd[s] : ag;
                dd[s] = d;
                if (d < mv) { mv = d; mi = s; }
            }
            wave_argmin(mv, mi);
            if (mv >= 0) break;
            if (lane == 0) sh_seed[K] = mi;
            __syncthreads();
        }
    }
    // rounds
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t m = lane; m < M; m += 64) prof[(uint64_t)k * M + m] = votes[(uint64_t)sh_seed[k] * M + m];
    for (uint32_t s = lane; s < S; s += 64) hap_of[s] = VC_POA_HAP_NONE;
    __syncthreads();
    for (uint32_t round = 0; round < hp.rounds; ++round) {
        bool moved = false;
        for (uint32_t s = lane; s < S; s += 64) {
            int32_t best = INT32_MIN;
            uint32_t bk = 0;
            for (uint32_t k = 0; k < K; ++k) {
                const int32_t ag = hap_agree(votes + (uint64_t)s * M, prof + (uint64_t)k * M, M);
                if (ag > best) { best = ag; bk = k; }
            }
            moved |= hap_of[s] != bk;
            hap_of[s] = (uint8_t)bk;
        }
        if (!__any(moved)) break;
        __syncthreads();
        for (uint32_t k = 0; k < K; ++k) {
            for (uint32_t m = lane; m < M; m += 64) {
                int32_t t = 0;
                for (uint32_t s = 0; s < S; ++s) if (hap_of[s] == k) t += votes[(uint64_t)s * M + m];
                prof[(uint64_t)k * M + m] = (int8_t)(t > 0 ? 1 : t < 0 ? -1 : 0);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    // small clusters, then the order
    if (lane < VC_POA_HAP_MAX) { sh_size[lane] = 0; sh_min[lane] = NONE; }
    __syncthreads();
    for (uint32_t s = lane; s < S; s += 64) { atomicAdd(&sh_size[hap_of[s]], 1u); atomicMin(&sh_min[hap_of[s]], s); }
    __syncthreads();
    bool any = false;
    for (uint32_t k = 0; k < K; ++k) any |= sh_size[k] >= hp.min_reads;
    for (uint32_t s = lane; s < S; s += 64) {
        const uint32_t k0 = hap_of[s];
        if (!any) { hap_of[s] = 0; continue; }
        if (sh_size[k0] >= hp.min_reads) continue;
        int32_t best = INT32_MIN;
        uint32_t bk = 0;
        for (uint32_t k = 0; k < K; ++k) {
            if (sh_size[k] < hp.min_reads) continue;
            const int32_t ag = hap_agree(votes + (uint64_t)s * M, prof + (uint64_t)k * M, M);
            if (ag > best) { best = ag; bk = k; }
        }
        hap_of[s] = (uint8_t)(bk | 0x80u);                             // (marked: the sizes below are still the old ones)
    }
    __syncthreads();
    if (lane == 0) {
        if (!any) { sh_k = 1; sh_map[0] = 0; for (uint32_t k = 1; k < K; ++k) sh_map[k] = NONE; sh_size[0] = S; sh_min[0] = 0; }
    }
    if (any) {
        __syncthreads();
        const bool keep = lane < K && sh_size[lane] >= hp.min_reads;
        __syncthreads();
        if (lane < VC_POA_HAP_MAX && !keep) { sh_size[lane] = 0; sh_min[lane] = NONE; }
        __syncthreads();
        for (uint32_t s = lane; s < S; s += 64) {
            if (!(hap_of[s] & 0x80u)) continue;
            const uint32_t k = hap_of[s] & 0x7Fu;
            hap_of[s] = (uint8_t)k;
            atomicAdd(&sh_size[k], 1u); atomicMin(&sh_min[k], s);
        }
        __syncthreads();
        if (lane == 0) {
            uint32_t n = 0;
            for (uint32_t k = 0; k < K; ++k) sh_map[k] = NONE;
            for (;;) {                                                 // selection by (size, largest first; then the smaller smallest label)
                uint32_t bk = NONE;
                for (uint32_t k = 0; k < K; ++k) {
                    if (sh_size[k] == 0 || sh_map[k] != NONE) continue;
                    if (bk == NONE || sh_size[k] > sh_size[bk] || (sh_size[k] == sh_size[bk] && sh_min[k] < sh_min[bk])) bk = k;
                }
                if (bk == NONE) break;
                sh_map[bk] = n++;
            }
            sh_k = n;
        }
    }
    __syncthreads();
    for (uint32_t s = lane; s < S; s += 64) hap_of[s] = (uint8_t)sh_map[hap_of[s]];
    if (lane == 0) { head[0] = sh_k; head[1] = M; }
    if (lane < K && sh_map[lane] != NONE) head[2 + sh_map[lane]] = sh_size[lane];
}

// one haplotype's restriction of the group's graph, and the bundle's scratch of this block (rule 8)
struct HapView {
    const LGraph& g;
    int64_t* scores;
    uint32_t *pred, *node_rank, *comp;
    const int64_t* wt;
    const uint32_t* outn;
    const uint8_t *eset, *nset;
    __device__ __forceinline__ bool node(uint32_t v) const { return nset[v] != 0; }
    __device__ __forceinline__ bool edge(uint32_t e) const { return eset[e] != 0; }
    __device__ __forceinline__ int64_t weight(uint32_t e) const { return wt[e]; }
    __device__ __forceinline__ uint32_t out_n(uint32_t v) const { return outn[v]; }
};

// The consensus of every haplotype (rule 8), one block per (group, haplotype) so that the haplotypes of a group run side by side,
// each on tables of its own behind the group's scratch: the restricted weights rebuilt from the members' paths -- a lane per step
// i, which finds the edge in the tail's out-list as add_edge did and adds w[i - 1] + w[i] --, the restricted out-degrees with a
// lane per edge, then the bundle on lane 0 as k_lg_apply runs the whole graph's.
__global__ __launch_bounds__(64) void k_lg_hapcons(LArgs a, LHap hp) {
    const uint32_t lane = threadIdx.x, q = blockIdx.x, k = blockIdx.y, groups = gridDim.x;
    LWin& W = a.win[a.list[q]];
    const LGraph& g = W.gr[W.cur];
    const uint32_t S = g.nseq, C = W.gr_cols, T = W.gr_path, N = g.n_nodes, E = g.n_edges;
    const HapBlock B = hap_block(S, C, N, hp.max_haps);
    const HapScratch X = hap_scratch(S, C, T, N, E, hp.max_haps);
    uint8_t* out = a.msa_out + a.hoff[q];
    uint8_t* scr = a.msa_out + a.hoff[groups + q];
    uint32_t* head = (uint32_t*)out;
    const uint8_t* hap_of = out + B.hap_of;
    const uint32_t *p_off = (const uint32_t*)(scr + X.p_off), *p_node = (const uint32_t*)(scr + X.p_node);
    uint8_t* mine = scr + X.per_hap + (uint64_t)k * X.hap_bytes;
    unsigned long long* wt = (unsigned long long*)(mine + X.h_wt);
    uint32_t* outn = (uint32_t*)(mine + X.h_outn);
    uint8_t *eset = mine + X.h_eset, *nset = mine + X.h_nset;
    if (S == 0 || k >= head[0]) return;                                    // no such haplotype, or the empty consensus: its length is zero already
    for (uint32_t e = lane; e < E; e += 64) { wt[e] = 0; eset[e] = 0; }
    for (uint32_t v = lane; v < N; v += 64) { outn[v] = 0; nset[v] = 0; }
    __syncthreads();
    for (uint32_t s = 0; s < S; ++s) {
        if (hap_of[s] != k) continue;
        const uint32_t sq = W.s0 + W.sq_member[s], p0 = p_off[s], len = p_off[s + 1] - p0;
        const bool uq = a.has_qual[sq] != 0;
        for (uint32_t i = lane; i < len; i += 64) {
            const uint32_t v = p_node[p0 + i];
            if (v >= N) continue;                                          // (every path entry is a node: the labels fill them all)
            nset[v] = 1;
            if (i == 0) continue;
            const uint32_t u = p_node[p0 + i - 1];
            if (u >= N) continue;
            const uint32_t w = weight_of(a, W, sq, i - 1, uq) + weight_of(a, W, sq, i, uq);
            for (uint32_t e = g.out_h[u]; e != NONE; e = g.nx_out[e]) {
                if (g.head[e] != v) continue;
                atomicAdd(&wt[e], (unsigned long long)w);
                eset[e] = 1;
                break;
            }
        }
    }
    __syncthreads();
    for (uint32_t e = lane; e < E; e += 64) if (eset[e]) atomicAdd(&outn[g.tail[e]], 1u);
    __syncthreads();
    if (lane != 0) return;
    const HapView V{g, (int64_t*)(mine + X.h_scores), (uint32_t*)(mine + X.h_pred), (uint32_t*)(mine + X.h_nrank), (uint32_t*)(mine + X.h_comp),
                    (const int64_t*)wt, outn, eset, nset};
    const uint32_t n = heaviest_bundle(g, V);
    uint8_t* cons = out + B.cons + (uint64_t)k * N;
    for (uint32_t i = 0; i < n; ++i) cons[i] = (uint8_t)W.decoder[g.code[V.comp[i]]];
    head[2 + VC_POA_HAP_MAX + k] = n;
}

}  // namespace
