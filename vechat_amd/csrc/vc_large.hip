// The large-graph path: the whole per-window algorithm on the device without the fast path's limits.
//
// The fast path (vc_api.hip) holds 16-bit node ids, LDS graph images and 16-bit adjacency offsets, so a window's graph stops at
// 59 968 nodes / 32 000 edges and a window with a longer layer stops at k_addaln's LDS notes; such windows come back
// VC_WIN_OVERFLOW.  vc_large_run computes them here: every id is 32 bits, every score int32 (int64 inside the horizontal scan),
// every table lives in HBM and is sized from what the window needs; a window whose tables fill is run again with larger ones.
// Slow by design: correctness counts here, not speed.  The device half -- the tables the kernels read, the graph functions and
// the kernels -- is vc_large_kernels.h; this file, the one translation unit, holds the host schedule and the C entries.
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
//     vc_poa_run_spans alone brings one window rule back, and only where the caller asks for it member by member: a later
//     member with a span (inclusive positions on sequence 0, which are node ids in a group built from nothing) is aligned against
//     Subgraph(begin, end) -- k_lg_prep extracts it into the other graph slot with schedule 0's subgraph(), one lane per group --,
//     k_lg_fwd / k_lg_back read its rows (view_of), and k_lg_apply maps the pairs back through W.map (UpdateAlignment) before
//     AddAlignment on the full graph; W.cur never flips.  The library applies no 1 % rule and no rank sort.  The spans travel in
//     LArgs::seq_begin / seq_end under LArgs::spans; a call without a span uploads none and is the plain call.  Both graph slots,
//     W.map, W.g2s, W.mark and W.stack have the full capacities in every schedule (layout), so spans change no allocation, and
//     a table that subgraph() fills (nodes, edges, aligned cells, stack) sets W.grow and the group runs again, as in the build.
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
//   k_lg_profile vc_poa_run_weighted with a profile only, one wave per finished group behind k_lg_msa<0>: the per-code counts and
//               the gaps of every consensus position (GenerateConsensus(&summary, true)) by a scatter over the edge labels;
//   k_lg_graph  vc_poa_run_graph only, one wave per finished group: <0> the counts of the group's graph tables, <1> the tables --
//               nodes, out-edges as CSR, aligned pairs, a path per sequence, the consensus path (spoa's GFA and dot output).
//   k_lg_load   vc_poa_run_from only, one wave per group behind k_lg_init: the group starts as a stored graph -- nodes, out-lists and
//               aligned lists from their CSR, in-lists and labels by replaying the paths in order; with a vc_poa_state_out
//               k_lg_graph<1> also writes every node's aligned list behind the group's block.
//   k_lg_hap    vc_poa_run_haplotypes only, one wave per finished group behind k_lg_graph<0>: sites, votes, seeds, rounds and the
//               order of the haplotypes (the rule: vechat_hip.h); k_lg_hapcons, a grid of (groups, max_haplotypes): the heaviest
//               bundle of the graph restricted to one haplotype's members, on weights rebuilt from their paths.
//   The query stage, vc_poa_run_align only (spoa's engine->Align(sequence, graph, &score) for sequences that are NOT added), on the
//   finished groups while their tables are resident; every (group, query) pair is a job (LJob) and independent of the others:
//   k_lg_rows   one lane per finished group: the graph half of k_lg_prep (graph_rows) once per group, without a next sequence;
//   k_lg_qfwd   <GM>, a grid of (jobs of the launch, strands), one wave per job and strand: k_lg_fwd's rows (fwd_rows) on the query
//               batch's bytes or their reverse-complement view (k_lg_views on the query batch);
//   k_lg_qback  <GM>, one lane per job: k_lg_back's walk (back_walk) into the job's own pair area of rows + length pairs;
//   k_lg_qpack  one wave per job: the pairs compact behind the host's prefix offsets, nodes and positions apart.
//   Assignment, vc_poa_run_assign only: every query of the call against every finished group, scores only, so no matrix is kept:
//   k_lg_slots  one lane per finished group behind k_lg_rows: the last reader of every row and, by a lowest-free-slot walk over
//               the ranks, the row's slot in a ring of n_slots rows (a row is kept only while a successor still reads it);
//   k_lg_sfwd   <GM>, a grid of (pairs of the launch, strands): fwd_rows with the row base taken from the slot, on a scratch of
//               n_slots x (len + 1) cells per plane; it leaves the score in the job;
//   k_lg_assign one lane per query: the scores of the chunk's pairs folded into the running best and second group (and, with
//               VC_POA_ASSIGN_SCORES, written into the dense table).
//   Correction, vc_poa_run_correct only (LArgs::correct): a group goes on after its build and its consensus through the prune
//   phases of schedule 0 -- prune + largest component, then num_prune - 1 rounds of one alignment per member and step with the
//   call's engine, add-weights, prune + largest component (k_lg_prep / k_lg_fwd / k_lg_back / k_lg_apply as above) --, and the
//   finished groups' members are then corrected side by side by the query stage's kernels: a job per member, the "query batch"
//   being the group batch itself and the type local (k_lg_rows, k_lg_qfwd, k_lg_qback), and
//   k_lg_correct <0> one wave per job: the pairs with a node, counted; <1> their nodes' bytes, compact behind the host's prefix
//               offsets (ballot and population count per tile of 64 pairs, a carried total) -- GenerateCorrectedSequence.
//
// Host schedule (Run, run_windows, run_group, lock_step): the windows or groups of a call run in host groups that fit the arena
// budget, one alignment of each per lock-step step, the forward passes in launches that fit the matrix budget (launch_loop).  What
// a vc_poa_* call hands out beside consensus and status comes from output stages (Stage): msa, profile, graph with the state
// table, correct and align.  A stage owns its tables and its per-call state and has four steps -- size, collect from a host group
// that finished while its tables are resident, assemble in window order with its log line, publish into the caller's out-struct --
// and the schedule walks the stages a call asks for without naming them.  Align and correct are one job stage (JobStage) with
// two kinds; graph and profile share their launch layout, every block in front of every scratch, and the copy that takes the
// blocks out.  The device buffers of a scope (DevMem), the device check and the knobs in MiB are vc_devutil.h's.
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
//                           "vc_large: correct jobs=J launches=K cells=C bytes=B" (vc_poa_run_correct: the members of the groups that
//                           finished, k_lg_qfwd launches of the final stage, their rows x columns, bytes copied out),
//                           "vc_large: assign groups=G queries=Q pairs=P launches=L slots_max=S ring_cells=C full_cells=F"
//                           (vc_poa_run_assign with queries: the groups and queries of the call, the pairs of the groups that
//                           finished, k_lg_sfwd launches, the largest n_slots of a group with a node, the int32 cells the launches
//                           stored -- slots x columns, every plane and strand -- and the cells k_lg_qfwd would have stored for the
//                           same pairs),
//                           "vc_large: state bytes=B" (vc_poa_run_from with a vc_poa_state_out: the bytes of the state tables, which
//                           the graph line does not count),
//                           "vc_large: load groups=G nodes=N edges=E paths=P bytes=B" (vc_poa_run_from with stored graphs: what was
//                           uploaded, once per call),
//                           "vc_large: spans members=M sub_rows=R full_rows=F" (vc_poa_run_spans with at least one span, before the
//                           "done" line: the members that were aligned against a subgraph, the rows of their forward passes summed,
//                           and the rows the same passes would have had against the whole graph; the rows count both strands'
//                           passes; every member counts once: a group that runs again with larger tables starts from zero, and
//                           a member whose matrix the device refused is not counted),
//                           "vc_large: profile launches=K bytes=B" (vc_poa_run_weighted with a profile: k_lg_profile launches, bytes
//                           copied out),
//                           "vc_large: haplotypes launches=K bytes=B" (vc_poa_run_haplotypes: k_lg_hap launches, bytes copied out),
//                           and at the end of a call "vc_large: done alignments=A cells=C" (forward passes of the build, their rows x
//                           columns summed; a regrown window's are counted again; vc_poa_run_strand counts both strands' passes;
//                           vc_poa_run_correct counts the rounds' passes too, not the final stage's).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "vechat_hip.h"

#include "vc_large_kernels.h"
#include "vc_devutil.h"

namespace {
// ------------------------------------------------------------------ host
using namespace vc_dev;                                // DevMem, ran(), env_mib(), check_device()

thread_local std::string g_err;
int fail(int rc, const char* m) { g_err = m; return rc; }

struct Caps { uint64_t NC, EC, AC, LC, SC, PC, nseq; };

// bytes of a window's tables, and (base != nullptr) the pointers into them
uint64_t layout(LWin* W, uint8_t* base, const Caps& c, bool labels, bool msa, bool stored = false) {
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
    if (msa && stored) { take(&x->sq_len, c.nseq); take(&x->sq_rev, c.nseq); }         // vc_poa_run_from: the stored paths' lengths and strands
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

// the development knobs of the header comment; false: VC_LARGE_CAPS does not parse
constexpr char kTables[] = "nealsp";                   // Knobs::shift order
struct Knobs { uint32_t shift[6] = {0, 0, 0, 0, 0, 0}; uint64_t arena = 0, mat = 0; bool log = false; };

bool read_knobs(Knobs& k) {
    k = Knobs{};
    k.arena = env_mib("VC_LARGE_ARENA_MB");
    k.mat = env_mib("VC_LARGE_MAT_MB");
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

// What a call wants beside consensus and status, and where each output goes (the caller's out-structs); vc_large_run's is empty.
struct PoaRequest {
    enum : uint32_t { MSA = 1, STRAND = 2, GRAPH = 4, ALIGN = 8, CORRECT = 16, ASSIGN = 32, HAPS = 64 };
    uint32_t required = 0;                             // the outputs the entry cannot do without; 0 leaves what an earlier call handed out alone
    vc_poa_msa_out* msa = nullptr;                     // rows, members and coverage as msa_flags say (0: n_groups only)
    vc_poa_strand_out* strand = nullptr;               // the strand flow, and its choices
    vc_poa_graph_out* graph = nullptr;                 // the graph tables, by the route LArgs::graph names (graph_route)
    const vc_batch* queries = nullptr;                 // vc_poa_run_align: the query batch and its output, with the align flags
    vc_poa_align_out* align = nullptr;
    uint32_t msa_flags = 0, route = 0, align_flags = 0;
    uint64_t nq = 0, nbytes = 0;                       // sequences and bytes of the query batch
    const vc_poa_prune_params* prune = nullptr;        // vc_poa_run_correct: the thresholds and rounds, and the corrected members
    vc_poa_correct_out* correct = nullptr;
    const vc_poa_graph_in* from = nullptr;             // vc_poa_run_from: the stored graphs the groups start as, and the state table beside the graph's
    vc_poa_state_out* state = nullptr;
    const vc_poa_span_in* spans = nullptr;             // vc_poa_run_spans with at least one span (check_spans leaves nullptr otherwise)
    const vc_poa_weight_in* weights = nullptr;         // vc_poa_run_weighted with at least one member of mode 1 or 2 (check_weights leaves nullptr otherwise)
    bool base_weights = false;                         // ... and at least one of mode 2
    vc_poa_profile_out* profile = nullptr;             // the per-code profile of every consensus
    vc_poa_assign_out* assign = nullptr;               // vc_poa_run_assign: `queries` are the queries of every group, and their best groups go here
    uint32_t assign_flags = 0;
    const vc_poa_hap_params* hap = nullptr;            // vc_poa_run_haplotypes: the rule's parameters, and the haplotypes of every group
    vc_poa_hap_out* haps = nullptr;
    bool rows() const { return msa_flags != 0; }                           // k_lg_msa runs
    bool columns() const { return rows() || profile != nullptr; }          // k_lg_msa<0> runs
    // the edges keep sequence labels, and the windows sq_begin / sq_member beside them
    bool keeps_labels() const { return msa_flags != 0 || graph != nullptr || profile != nullptr || haps != nullptr; }
    uint32_t strands() const { return strand ? 2 : 1; }                    // forward passes per alignment of the build
    bool has_queries() const { return nq != 0; }                           // the query stage runs (a call without a query is the call without it)
    bool query_pairs() const { return (align_flags & VC_POA_ALIGN_PAIRS) != 0; }
    uint32_t query_strands() const { return (align_flags & VC_POA_ALIGN_STRANDS) || (assign_flags & VC_POA_ASSIGN_STRANDS) ? 2 : 1; }
    bool assign_scores() const { return (assign_flags & VC_POA_ASSIGN_SCORES) != 0; }
};

// an empty table is still a pointer
template <class T> T* table(std::vector<T>& v) { v.reserve(1); return v.data(); }

// ------------------------------------------------------------------ the host schedule
// One call of vc_large_run / vc_poa_run*: the batch on the device (seq_begin / seq_end only with spans), windows in flight in
// groups that fit the arena budget, one alignment of each per lock-step step with the forward passes in launches that fit the
// matrix budget, and a window whose table filled run again with larger tables.  `a` holds the scores and the schedule, `q` what
// the call wants beside the consensus, `stages` the output stages that deliver it (below; they keep their own state).
struct Stage;
struct Run {
    LArgs a;
    const vc_batch* b;
    std::vector<Caps>& caps;
    const Knobs& kn;
    const PoaRequest& q;
    bool labels;                                       // the racon-linear overload's coverage reads them too
    uint32_t nw;
    uint64_t nseq_all, nbytes;
    uint64_t arena_budget = 0, mat_budget = 0;
    uint64_t planes = 1;                               // int32 planes per matrix cell
    uint32_t ns = 1;                                   // forward passes, and matrices, per alignment: one per strand
    std::vector<uint32_t> pending;                     // windows still to run, in order
    std::vector<std::vector<uint8_t>> out;             // per window: the consensus
    std::vector<uint8_t> status;
    uint64_t n_align = 0, n_cells = 0;                 // forward passes run (VC_LARGE_LOG's "done" line)
    // vc_poa_run_spans (the "spans" line), per group: members aligned to a subgraph, the rows of their forward passes, the whole
    // graph's rows for the same passes.  A group that runs again starts from zero, so every member counts once
    struct SpanCount { uint64_t members = 0, rows = 0, full = 0; };
    std::vector<SpanCount> sp_of;
    LLoad load{};                                      // vc_poa_run_from: the stored graphs on the device
    std::vector<Stage*> stages;                        // the output stages of this call, in their order (Outputs::active)
};

// the windows in flight together: their ids, their tables in the arena, their LWin here and on the device
struct Group {
    std::vector<uint32_t> ids;
    std::vector<uint64_t> aoff;
    uint64_t abytes = 0;
    std::vector<LWin> hw;
    LWin* d_win = nullptr;
    uint32_t* d_list = nullptr;                        // the windows of one launch (k_lg_fwd / k_lg_back / k_lg_msa<1>), as indices into d_win;
                                                       // k_lg_load alone is given the ids of all windows in flight in the BATCH here ...
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

// vc_poa_run_align, vc_poa_run_assign: the query batch on the device -- offsets and bytes, and with VC_POA_ALIGN_STRANDS /
// VC_POA_ASSIGN_STRANDS its reverse-complement view (k_lg_views on the query batch's arrays: no quality, no round trip) -- once per call
int upload_queries(Run& R, DevMem& mem) {
    const PoaRequest& A = R.q;
    uint64_t* d_off = nullptr;
    uint8_t *d_b = nullptr, *d_rc = nullptr;
    const bool strands = A.query_strands() == 2;
    bool ok = mem.alloc(&d_off, A.nq + 1, A.queries->seq_off) && mem.alloc(&d_b, A.nbytes, A.queries->bases) && (!strands || mem.alloc(&d_rc, A.nbytes));
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

// vc_poa_run_from: the stored graphs on the device, once per call -- the arrays as given (check_from has passed them) and the
// decoder of every group: its bytes in order of first appearance along the paths in order, as add_alignment met them (then any
// byte of a node that no path visits, which a graph this library wrote does not have) -- and the call's log line
int upload_stored(Run& R, DevMem& mem) {
    const vc_poa_graph_in* f = R.q.from;
    const uint32_t ng = f->n_groups;
    const uint64_t NN = f->node_off[ng], PP = f->path_first[ng], EE = f->out_off[NN + ng - 1], AA = f->al_off[NN + ng - 1], TT = f->path_off[PP];
    std::vector<uint8_t> dec(256ull * ng, 0);
    std::vector<uint32_t> n_codes(ng, 0);
    for (uint32_t w = 0; w < ng; ++w) {
        bool seen[256] = {};
        uint8_t* d = dec.data() + 256ull * w;
        auto meet = [&](uint8_t c) { if (!seen[c]) { seen[c] = true; d[n_codes[w]++] = c; } };
        const uint64_t nb = f->node_off[w];
        for (uint64_t k = f->path_off[f->path_first[w]]; k < f->path_off[f->path_first[w + 1]]; ++k) meet(f->node_base[nb + f->path_node[k]]);
        for (uint64_t v = 0; v < f->n_nodes[w]; ++v) meet(f->node_base[nb + v]);
    }
    LLoad& L = R.load;
    if (!mem.alloc(&L.n_nodes, ng, f->n_nodes) || !mem.alloc(&L.node_off, ng + 1, f->node_off) || !mem.alloc(&L.node_base, NN, f->node_base) ||
        !mem.alloc(&L.rank_to_node, NN, f->rank_to_node) || !mem.alloc(&L.out_off, NN + ng, f->out_off) || !mem.alloc(&L.edge_head, EE, f->edge_head) ||
        !mem.alloc(&L.edge_weight, EE, f->edge_weight) || !mem.alloc(&L.al_off, NN + ng, f->al_off) || !mem.alloc(&L.al_node, AA, f->al_node) ||
        !mem.alloc(&L.path_first, ng + 1, f->path_first) || !mem.alloc(&L.path_member, PP, f->path_member) ||
        !mem.alloc(&L.path_reversed, PP, f->path_reversed) || !mem.alloc(&L.path_off, PP + 1, f->path_off) || !mem.alloc(&L.path_node, TT, f->path_node) ||
        !mem.alloc(&L.dec, dec.size(), dec.data()) || !mem.alloc(&L.n_codes, ng, n_codes.data()))
        return fail(VC_ERR_HIP, "device allocation or copy of the stored graphs failed");
    if (R.kn.log) {
        const uint64_t bytes = 4ull * ng + 8 * (ng + 1) + NN + 4 * NN + 2 * 8 * (NN + ng) + 4 * EE + 8 * EE + 4 * AA + 8 * (ng + 1) + 4 * PP + PP +
                               8 * (PP + 1) + 4 * TT + dec.size() + 4ull * ng;
        std::fprintf(stderr, "vc_large: load groups=%u nodes=%llu edges=%llu paths=%llu bytes=%llu\n", ng, (unsigned long long)NN,
                     (unsigned long long)EE, (unsigned long long)PP, (unsigned long long)bytes);
    }
    return VC_OK;
}

// The windows in flight next: as many of the pending ones as the arena budget holds, in order (at least one; a window the device
// cannot hold at all is refused).  G.ids is empty when every pending window was refused.
void next_group(Run& R, Group& G) {
    std::vector<uint32_t> rest;
    for (uint32_t w : R.pending) {
        const uint64_t need = layout(nullptr, nullptr, R.caps[w], R.labels, R.q.keeps_labels(), R.q.from != nullptr);
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
        layout(&W, arena + G.aoff[k], R.caps[w], R.labels, R.q.keeps_labels(), R.q.from != nullptr);
        if (const vc_poa_graph_in* f = R.q.from) { W.n_old = (uint32_t)(f->path_first[w + 1] - f->path_first[w]); W.m0 = f->n_members[w]; }
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

// The launches of one stage over `items`: consecutive items while their sizes fit the budget (pack_launch), room for them in the
// matrix buffer (`unit` bytes per unit of size), list and hoff (which place() may lay out anew) on the device, then the stage's
// body(f, list, hoff, total, buffer) with f = a + list + hoff, which launches and copies out.  A single item the device has no room
// for goes to refuse(item) and the loop goes on; several are the error no_room.  Every launch that ran is counted.
struct StageErrors { const char *no_room, *no_upload; };
const auto as_packed = [](const std::vector<uint32_t>&, std::vector<uint64_t>&) {};

template <class Size, class Place, class Refuse, class Body>
int launch_loop(const LArgs& a, const std::vector<uint32_t>& items, uint64_t budget, uint64_t unit, uint32_t* d_list, uint64_t* d_hoff,
                const StageErrors& err, uint64_t& launches, Size size, Place place, Refuse refuse, Body body) {
    std::vector<uint32_t> list;
    std::vector<uint64_t> hoff;
    LArgs f = a;
    f.list = d_list; f.hoff = d_hoff;
    for (size_t k0 = 0; k0 < items.size();) {
        uint64_t total;
        k0 = pack_launch(items, k0, budget, size, list, hoff, total);
        place(list, hoff);
        void* buf = cached(g_cache.mat, total * unit);
        if (!buf) {
            if (list.size() > 1) return fail(VC_ERR_HIP, err.no_room);
            if (const int rc = refuse(list[0])) return rc;
            continue;
        }
        if (hipMemcpy(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_hoff, hoff.data(), hoff.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(VC_ERR_HIP, err.no_upload);
        if (const int rc = body(f, list, hoff, total, buf)) return rc;
        launches++;
    }
    return VC_OK;
}

// group k finished and no stage has refused it: its outputs may be collected
bool finished(const Run& R, const Group& G, uint32_t k) {
    return !G.hw[k].grow && G.hw[k].status == VC_WIN_OK && R.status[G.ids[k]] == VC_WIN_OK;
}
std::vector<uint32_t> finished(const Run& R, const Group& G) {
    std::vector<uint32_t> fin;
    for (uint32_t k = 0; k < G.ids.size(); ++k) if (finished(R, G, k)) fin.push_back(k);
    return fin;
}

// launch(gm) with the gap model LArgs::gaps as a constant: the <GM> of k_lg_fwd / k_lg_back and of the query stage's kernels
template <class Launch>
void with_gap_model(uint32_t gaps, Launch launch) {
    if (gaps == 0) launch(std::integral_constant<uint32_t, 0>{});
    else if (gaps == 1) launch(std::integral_constant<uint32_t, 1>{});
    else launch(std::integral_constant<uint32_t, 2>{});
}

template <uint32_t GM>
void launch_align(const LArgs& f, uint32_t nl, uint32_t ns) {
    hipLaunchKernelGGL(k_lg_fwd<GM>, dim3(nl, ns), dim3(64), 0, 0, f);
    hipLaunchKernelGGL(k_lg_back<GM>, dim3((nl + 63) / 64), dim3(64), 0, 0, f, nl);
}

// The forward passes and backtracks of one step, over the windows `act` that have an alignment: their matrices in launches that
// fit the budget (in int32 cells of every plane and strand); a matrix the device cannot hold takes its window out.
bool align_step(Run& R, Group& G, const std::vector<uint32_t>& act) {
    static const char* const failed = "a large-graph kernel failed";
    uint64_t launches = 0, over = 0;
    auto matrix_cells = [&](uint32_t k) { return ((uint64_t)G.hw[k].rows + 1) * ((uint64_t)G.hw[k].qlen + 1) * R.planes * R.ns; };
    auto refuse = [&](uint32_t k) -> int {
        LWin& W = G.hw[k];
        W.phase = PH_DONE; W.status = VC_WIN_OVERFLOW; W.rows = 0;
        return hipMemcpy(G.d_win + k, &W, sizeof(LWin), hipMemcpyHostToDevice) == hipSuccess ? VC_OK : fail(VC_ERR_HIP, failed);
    };
    auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>&, uint64_t cells, void* H) -> int {
        const uint32_t nl = (uint32_t)list.size();
        f.H = (int32_t*)H;
        with_gap_model(f.gaps, [&](auto gm) { launch_align<decltype(gm)::value>(f, nl, R.ns); });
        if (!ran()) return fail(VC_ERR_HIP, failed);
        for (const uint32_t k : list) R.n_cells += (uint64_t)G.hw[k].rows * G.hw[k].qlen * R.ns;
        R.n_align += (uint64_t)nl * R.ns;
        if (cells * 4 > R.mat_budget) over++;
        return VC_OK;
    };
    if (launch_loop(R.a, act, R.mat_budget / 4, 4, G.d_list, G.d_hoff, {failed, failed}, launches, matrix_cells, as_packed, refuse, body)) return false;
    if (R.kn.log && launches > 1) std::fprintf(stderr, "vc_large: step launches=%llu over=%llu\n", (unsigned long long)launches, (unsigned long long)over);
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
    if (ok && R.q.from) {                                                  // every group starts as its stored graph
        LArgs f = a;
        f.list = G.d_list;
        ok = hipMemcpy(G.d_list, G.ids.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) { hipLaunchKernelGGL(k_lg_load, dim3(n), dim3(64), 0, 0, f, R.load); ok = hipGetLastError() == hipSuccess; }
    }
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
        if (a.spans) {
            // the "spans" line, per group: a member whose forward passes ran on a subgraph (a refused matrix has left rows == 0)
            for (const uint32_t k : act) {
                const LWin& W = G.hw[k];
                if (!W.rows || !W.sub) continue;
                Run::SpanCount& c = R.sp_of[G.ids[k]];
                c.members++; c.rows += (uint64_t)W.rows * R.ns; c.full += (uint64_t)W.gr[W.cur].n_nodes * R.ns;
            }
        }
        if (a.wmode) hipLaunchKernelGGL(k_lg_apply<true>, lanes, dim3(64), 0, 0, a);
        else hipLaunchKernelGGL(k_lg_apply<false>, lanes, dim3(64), 0, 0, a);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && R.q.columns()) hipLaunchKernelGGL(k_lg_msa<0>, dim3(n), dim3(64), 0, 0, a);
    if (ok && (R.q.graph || R.q.haps)) hipLaunchKernelGGL(k_lg_graph<0>, dim3(n), dim3(64), 0, 0, a);   // (the haplotype stage sizes itself from the same counts)
    ok = ok && hipGetLastError() == hipSuccess;
    return ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(G.hw.data(), G.d_win, n * sizeof(LWin), hipMemcpyDeviceToHost) == hipSuccess;
}

// a table of window w filled (W.grow): larger tables, and the window runs again unless they outgrow the 32-bit ids
void regrow(Run& R, uint32_t w, const LWin& W) {
    Caps& c = R.caps[w];
    if (!R.sp_of.empty()) R.sp_of[w] = Run::SpanCount{};                   // the group runs again: its members are counted then
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

// ------------------------------------------------------------------ the output stages
// What a vc_poa_* call hands out beside consensus and status, one stage per output: msa, profile, graph (with the state table),
// correct and align.  A stage owns the tables it hands out and what it keeps per window during a call, and has four steps:
// size() for the call; collect() from the groups of a Group that finished, while their tables are resident; assemble() in window
// order, with the stage's log line; publish() into the caller's out-struct, where the call has one.  The stages live in g_out
// (below), so their tables stay valid until the next call that has an output of its own, or vc_large_release.
struct Stage {
    virtual ~Stage() = default;
    virtual void size(const Run& R) = 0;
    virtual int collect(Run& R, Group& G) = 0;
    virtual void assemble(const Run& R) = 0;
    virtual void publish(const PoaRequest& q, const vc_batch* b) = 0;
};

int refuse_group(Run& R, uint32_t w) { R.status[w] = VC_WIN_OVERFLOW; R.out[w].clear(); return VC_OK; }   // a stage has no room for the one group w

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

// The alignments and the coverage (vc_poa_msa_out): blocks laid out in the matrix buffer (free after the last step), in launches
// that fit the matrix budget, each copied out at once, straight into `rows`.
struct MsaStage : Stage {
    std::vector<uint32_t> n_rows, row_size, row_member, coverage;
    std::vector<uint64_t> row_off, member_off;
    std::vector<uint8_t> rows;
    std::vector<std::vector<uint32_t>> mem_of, cov_of; // until assemble(), per window: the row members and the coverage
    uint64_t launches = 0;

    void size(const Run& R) override {
        mem_of.resize(R.nw); cov_of.resize(R.nw);
        n_rows.assign(R.nw, 0); row_size.assign(R.nw, 0); row_off.assign(R.nw, 0); member_off.assign(R.nw + 1, 0);
    }
    int collect(Run& R, Group& G) override {
        const LArgs& a = R.a;
        auto block_bytes = [&](uint32_t k) { return msa_block(G.hw[k], a.msa).bytes; };
        auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>& hoff, uint64_t bytes, void* dout) -> int {
            const uint32_t nl = (uint32_t)list.size();
            const uint64_t at = rows.size();
            f.msa_out = (uint8_t*)dout;
            hipLaunchKernelGGL(k_lg_msa<1>, dim3(nl), dim3(64), 0, 0, f);
            bool ok = hipGetLastError() == hipSuccess;
            rows.resize(at + bytes);
            ok = ok && hipMemcpy(rows.data() + at, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess;
            if (!ok) return fail(VC_ERR_HIP, "the alignment-row kernel or its copy failed");
            for (uint32_t q = 0; q < nl; ++q) {
                const LWin& W = G.hw[list[q]];
                const uint32_t w = G.ids[list[q]];
                const MsaBlock B = msa_block(W, a.msa);
                const uint8_t* blk = rows.data() + at + hoff[q];
                n_rows[w] = W.msa_rows; row_size[w] = W.row_size; row_off[w] = at + hoff[q];
                mem_of[w].resize(W.msa_rows);
                if (W.msa_rows) std::memcpy(mem_of[w].data(), blk + B.mem_at, 4ull * W.msa_rows);
                if (a.msa & VC_POA_COVERAGE) {
                    cov_of[w].resize(W.cons_n);
                    if (W.cons_n) std::memcpy(cov_of[w].data(), blk + B.cov_at, 4ull * W.cons_n);
                }
            }
            return VC_OK;
        };
        return launch_loop(a, finished(R, G), R.mat_budget, 1, G.d_list, G.d_hoff,
                           {"device allocation of the alignment rows failed", "the alignment-row kernel or its copy failed"}, launches,
                           block_bytes, as_packed, [&](uint32_t k) { return refuse_group(R, G.ids[k]); }, body);
    }
    // the per-row and per-base tables in window order
    void assemble(const Run& R) override {
        member_off[0] = 0;
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] != VC_WIN_OK) { n_rows[w] = 0; row_size[w] = 0; mem_of[w].clear(); cov_of[w].clear(); }
            row_member.insert(row_member.end(), mem_of[w].begin(), mem_of[w].end());
            member_off[w + 1] = row_member.size();
            if (R.a.msa & VC_POA_COVERAGE) {
                cov_of[w].resize(R.out[w].size());
                coverage.insert(coverage.end(), cov_of[w].begin(), cov_of[w].end());
            }
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: msa launches=%llu bytes=%llu\n", (unsigned long long)launches, (unsigned long long)rows.size());
    }
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_msa_out* o = q.msa;
        if (!o) return;
        o->n_groups = b->n_windows;
        if (!q.rows() || !b->n_windows) return;                            // without flags: n_groups only
        o->n_rows = n_rows.data(); o->row_size = row_size.data(); o->row_off = row_off.data();
        o->member_off = member_off.data(); o->row_member = row_member.data();
        o->rows = rows.data(); o->rows_bytes = rows.size();
        if (o->flags & VC_POA_COVERAGE) o->coverage = coverage.data();
    }
};

// The launch layout of the stages that copy a block per group out and leave a scratch per group behind (graph, profile): every
// block, then every scratch -- hoff[q] and hoff[groups + q] for group list[q] -- so that one copy takes the blocks out.  Returns
// the blocks' bytes.
template <class Block, class Scratch>
uint64_t blocks_first(const std::vector<uint32_t>& list, std::vector<uint64_t>& hoff, Block block_of, Scratch scratch_of) {
    const uint32_t nl = (uint32_t)list.size();
    uint64_t blocks = 0;
    hoff.assign(2 * (size_t)nl, 0);
    for (uint32_t q = 0; q < nl; ++q) { hoff[q] = blocks; blocks += block_of(list[q]); }
    uint64_t at = blocks;
    for (uint32_t q = 0; q < nl; ++q) { hoff[nl + q] = at; at += scratch_of(list[q]); }
    return blocks;
}

// ... and that copy: the blocks in front of dout into `host`, then block q into the bytes that part_of(q) names
template <class Part>
bool blocks_out(const void* dout, uint64_t blocks, const std::vector<uint64_t>& hoff, uint32_t nl, std::vector<uint8_t>& host, Part part_of) {
    host.resize(blocks);
    if (blocks && hipMemcpy(host.data(), dout, blocks, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (uint32_t q = 0; q < nl; ++q) part_of(q).assign(host.begin() + hoff[q], host.begin() + (q + 1 < nl ? hoff[q + 1] : blocks));
    return true;
}

// The per-code profile of every consensus (vc_poa_profile_out): a block (counts, then codes) and a scratch per group in the matrix
// buffer.  The groups' columns are k_lg_msa<0>'s, of the same lock_step.
struct ProfileStage : Stage {
    std::vector<uint32_t> n_codes, counts;
    std::vector<uint64_t> code_off, prof_off;
    std::vector<uint8_t> codes;
    uint64_t bytes = 0;                                // copied out of the device
    std::vector<std::vector<uint8_t>> blk;             // until assemble(), per window: its block and its code count
    std::vector<uint32_t> nc_of;
    uint64_t launches = 0;

    void size(const Run& R) override { blk.resize(R.nw); nc_of.assign(R.nw, 0); }
    int collect(Run& R, Group& G) override {
        auto block_of = [&](uint32_t k) { return profile_block(G.hw[k].num_codes, G.hw[k].cons_n).bytes; };
        auto scratch_of = [&](uint32_t k) { return profile_scratch(G.hw[k].gr[G.hw[k].cur].nseq, G.hw[k].gr_cols).bytes; };
        uint64_t blocks = 0;
        std::vector<uint8_t> host;
        auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>& hoff, uint64_t, void* dout) -> int {
            const uint32_t nl = (uint32_t)list.size();
            f.msa_out = (uint8_t*)dout;
            hipLaunchKernelGGL(k_lg_profile, dim3(nl), dim3(64), 0, 0, f);
            auto part_of = [&](uint32_t q) -> std::vector<uint8_t>& {
                const uint32_t w = G.ids[list[q]];
                nc_of[w] = G.hw[list[q]].num_codes;
                return blk[w];
            };
            if (hipGetLastError() != hipSuccess || !blocks_out(dout, blocks, hoff, nl, host, part_of))
                return fail(VC_ERR_HIP, "the profile kernel or its copy failed");
            bytes += blocks;
            return VC_OK;
        };
        return launch_loop(R.a, finished(R, G), R.mat_budget, 1, G.d_list, G.d_hoff,
                           {"device allocation of the profile blocks failed", "the profile kernel or its copy failed"}, launches,
                           [&](uint32_t k) { return block_of(k) + scratch_of(k); },
                           [&](const std::vector<uint32_t>& list, std::vector<uint64_t>& hoff) { blocks = blocks_first(list, hoff, block_of, scratch_of); },
                           [&](uint32_t k) { return refuse_group(R, G.ids[k]); }, body);
    }
    // the tables in window order (a group that was not computed has no code and an empty block)
    void assemble(const Run& R) override {
        code_off.assign(1, 0);
        for (uint32_t w = 0; w < R.nw; ++w) {
            const uint32_t nc = R.status[w] == VC_WIN_OK && !blk[w].empty() ? nc_of[w] : 0;
            const uint64_t Cn = R.out[w].size();
            n_codes.push_back(nc);
            prof_off.push_back(counts.size());
            if (nc) {
                const uint32_t* c = (const uint32_t*)blk[w].data();
                counts.insert(counts.end(), c, c + (uint64_t)(nc + 1) * Cn);
                const uint8_t* cd = blk[w].data() + profile_block(nc, Cn).codes;
                codes.insert(codes.end(), cd, cd + nc);
            }
            code_off.push_back(codes.size());
            blk[w] = std::vector<uint8_t>{};
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: profile launches=%llu bytes=%llu\n", (unsigned long long)launches, (unsigned long long)bytes);
    }
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_profile_out* po = q.profile;
        if (!po) return;
        po->n_groups = b->n_windows;
        if (!b->n_windows) return;
        po->n_codes = n_codes.data(); po->code_off = code_off.data(); po->codes = table(codes);
        po->prof_off = prof_off.data(); po->counts = table(counts);
    }
};

// The graph tables (vc_poa_graph_out) and, with a vc_poa_state_out, the state table beside them: a block and a scratch per group
// in the matrix buffer; k_lg_graph<1> writes a group's state table behind its block, so the same copy takes it out.
struct GraphStage : Stage {
    std::vector<uint32_t> n_nodes, rank_to_node, edge_head, aligned_a, aligned_b, path_member, path_node, cons_node;
    std::vector<uint64_t> node_off, out_off, aligned_off, path_first, path_off;
    std::vector<uint8_t> node_base, path_reversed;
    std::vector<int32_t> node_cons_pos;
    std::vector<int64_t> edge_weight;
    uint64_t bytes = 0;                                // copied out of the device
    std::vector<uint64_t> al_off;                      // vc_poa_state_out
    std::vector<uint32_t> al_node;
    uint64_t state_copied = 0;                         // its bytes, which `bytes` does not count
    // until assemble(), per window: its block of k_lg_graph<1> and the counts that lay it out (A: cells of the state table behind it)
    struct Part { uint32_t N = 0, E = 0, P = 0, S = 0, T = 0, Cn = 0, A = 0; std::vector<uint8_t> blk; };
    std::vector<Part> part;
    uint64_t launches = 0;

    void size(const Run& R) override { part.resize(R.nw); }
    int collect(Run& R, Group& G) override {
        const LArgs& a = R.a;
        auto counts_of = [&](uint32_t k) {
            const LWin& W = G.hw[k];
            const LGraph& g = W.gr[W.cur];
            Part p;
            p.N = g.n_nodes; p.E = g.n_edges; p.P = g.n_al / 2; p.S = g.nseq; p.T = W.gr_path; p.Cn = W.cons_n; p.A = a.state ? g.n_al : 0;
            return p;
        };
        auto state_of = [&](uint32_t k) { const Part p = counts_of(k); return a.state ? state_bytes(p.N, p.A) : 0; };
        auto block_of = [&](uint32_t k) { const Part p = counts_of(k); return graph_block(p.N, p.E, p.P, p.S, p.T, p.Cn).bytes + state_of(k); };
        auto scratch_of = [&](uint32_t k) { return a.graph == 1 ? graph_scratch_bytes(G.hw[k].gr[G.hw[k].cur].nseq, G.hw[k].gr_cols) : 0; };
        uint64_t blocks = 0;
        std::vector<uint8_t> host;
        auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>& hoff, uint64_t, void* dout) -> int {
            const uint32_t nl = (uint32_t)list.size();
            f.msa_out = (uint8_t*)dout;
            hipLaunchKernelGGL(k_lg_graph<1>, dim3(nl), dim3(64), 0, 0, f);
            auto part_of = [&](uint32_t q) -> std::vector<uint8_t>& {
                Part& p = part[G.ids[list[q]]];
                p = counts_of(list[q]);
                return p.blk;
            };
            if (hipGetLastError() != hipSuccess || !blocks_out(dout, blocks, hoff, nl, host, part_of))
                return fail(VC_ERR_HIP, "the graph kernel or its copy failed");
            uint64_t st = 0;                                               // the state tables lie in the same copy: counted apart
            for (const uint32_t k : list) st += state_of(k);
            bytes += blocks - st;
            state_copied += st;
            return VC_OK;
        };
        return launch_loop(a, finished(R, G), R.mat_budget, 1, G.d_list, G.d_hoff,
                           {"device allocation of the graph tables failed", "the graph kernel or its copy failed"}, launches,
                           [&](uint32_t k) { return block_of(k) + scratch_of(k); },
                           [&](const std::vector<uint32_t>& list, std::vector<uint64_t>& hoff) { blocks = blocks_first(list, hoff, block_of, scratch_of); },
                           [&](uint32_t k) { return refuse_group(R, G.ids[k]); }, body);
    }
    // the tables in window order, every offset rebased from its block to the batch
    void assemble(const Run& R) override {
        auto put = [](auto& dst, const Part& p, uint64_t at, uint64_t n) {
            using T = typename std::remove_reference_t<decltype(dst)>::value_type;
            const T* src = (const T*)(p.blk.data() + at);
            dst.insert(dst.end(), src, src + n);
        };
        node_off.assign(1, 0); aligned_off.assign(1, 0); path_first.assign(1, 0); path_off.assign(1, 0);
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] != VC_WIN_OK) part[w] = Part{};
            const Part& p = part[w];
            const GraphBlock B = graph_block(p.N, p.E, p.P, p.S, p.T, p.Cn);
            const uint64_t e0 = edge_head.size(), t0 = path_node.size(), c0 = al_node.size();
            n_nodes.push_back(p.N);
            if (!p.blk.empty()) {
                put(node_base, p, B.base, p.N); put(node_cons_pos, p, B.cons_pos, p.N); put(rank_to_node, p, B.rank, p.N);
                put(edge_head, p, B.head, p.E); put(edge_weight, p, B.weight, p.E);
                put(aligned_a, p, B.al_a, p.P); put(aligned_b, p, B.al_b, p.P);
                put(path_member, p, B.member, p.S); put(path_reversed, p, B.rev, p.S); put(path_node, p, B.p_node, p.T);
                put(cons_node, p, B.cons_node, p.Cn);
                const uint32_t* oo = (const uint32_t*)(p.blk.data() + B.out_off);
                for (uint32_t v = 0; v <= p.N; ++v) out_off.push_back(e0 + oo[v]);
                const uint32_t* po = (const uint32_t*)(p.blk.data() + B.p_off);
                for (uint32_t k = 1; k <= p.S; ++k) path_off.push_back(t0 + po[k]);
                if (R.a.state) {                                           // the state table lies behind the block
                    const uint32_t* ao = (const uint32_t*)(p.blk.data() + B.bytes);
                    for (uint32_t v = 0; v <= p.N; ++v) al_off.push_back(c0 + ao[v]);
                    put(al_node, p, B.bytes + state_list_at(p.N), p.A);
                }
            } else {
                out_off.push_back(e0);         // a group without a block has no node and no path: its one out_off entry
                if (R.a.state) al_off.push_back(c0);
            }
            node_off.push_back(node_base.size());
            aligned_off.push_back(aligned_a.size());
            path_first.push_back(path_member.size());
            part[w] = Part{};
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: graph launches=%llu bytes=%llu\n", (unsigned long long)launches, (unsigned long long)bytes);
        if (R.kn.log && R.a.state) std::fprintf(stderr, "vc_large: state bytes=%llu\n", (unsigned long long)state_copied);
    }
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_graph_out* go = q.graph;
        if (!go) return;
        go->n_groups = b->n_windows;
        if (!b->n_windows) return;
        go->n_nodes = table(n_nodes); go->node_off = node_off.data(); go->node_base = table(node_base);
        go->node_cons_pos = table(node_cons_pos); go->rank_to_node = table(rank_to_node);
        go->out_off = out_off.data(); go->edge_head = table(edge_head); go->edge_weight = table(edge_weight);
        go->aligned_off = aligned_off.data(); go->aligned_a = table(aligned_a); go->aligned_b = table(aligned_b);
        go->path_first = path_first.data(); go->path_member = table(path_member); go->path_reversed = table(path_reversed);
        go->path_off = path_off.data(); go->path_node = table(path_node);
        go->cons_node = table(cons_node);
        go->bytes = bytes;
        if (vc_poa_state_out* st = q.state) { st->al_off = al_off.data(); st->al_node = table(al_node); st->bytes = state_copied; }
    }
};

template <uint32_t GM>
void launch_query(const LArgs& f, uint32_t nl, uint32_t ns, bool pairs) {
    hipLaunchKernelGGL(k_lg_qfwd<GM>, dim3(nl, ns), dim3(64), 0, 0, f);
    if (pairs) hipLaunchKernelGGL(k_lg_qback<GM>, dim3((nl + 63) / 64), dim3(64), 0, 0, f, nl);
}

// The job stage behind align and correct: sequences aligned against the finished graph of their group, while its tables are
// resident, and not added to it -- the group's queries (align) or its own members (correct).  Every (group, sequence) pair is a
// job (LJob), independent of the others, so a launch holds as many as fit the matrix budget.  What a job hands back beside status
// and scores is NP planes of T: the node and the position of every pair (align), the corrected bytes (correct).
template <class T, uint32_t NP>
struct JobStage : Stage {
    // one entry per sequence of the source batch (score_rev and reversed: with both strands only); off: where its entries of every plane begin
    std::vector<uint8_t> status, reversed;
    std::vector<int32_t> score, score_rev;
    std::vector<uint64_t> off;
    std::vector<T> plane[NP];
    uint64_t bytes = 0;                                // copied out of the device
    // until assemble(): per collect() the packed planes one behind the other, per sequence which of them and where in a plane
    std::vector<std::vector<T>> part;
    std::vector<uint32_t> part_of, count;
    std::vector<uint64_t> first;
    uint64_t n_jobs = 0, launches = 0, n_cells = 0;    // the log line's counts

    // What the two stages differ in.  The messages: allocation, k_lg_rows, a launch's kernels, launch_loop's two, the count kernel
    // or the copy of the job table, the pack kernel or its copy; then the log line.
    struct Kind {
        LArgs a;                                       // the call's, with the source batch as the query batch
        const vc_batch* src;                           // the jobs of group w: the sequences of src's window w
        uint32_t ns;                                   // strands per job
        bool pairs;                                    // the backtrack runs, and the planes are filled
        uint32_t LJob::*n;                             // a job's entries per plane ...
        void (*count)(const LArgs& a, uint32_t nj);    // ... and the kernel that counts them before the job table comes back (nullptr: none)
        void (*pack)(LArgs a, T* d_out, uint32_t nj, uint64_t total);      // the kernel that packs every job's entries behind its pair_off
        const char *no_jobs, *no_rows, *no_kernel;
        StageErrors launch;
        const char *no_count, *no_pack, *log;
    };
    virtual Kind kind(const Run& R) const = 0;

    void size(const Run& R) override {
        const Kind K = kind(R);
        const uint64_t n = K.src->win_seq_off[R.nw];
        status.assign(n, VC_WIN_OVERFLOW); score.assign(n, 0);
        if (K.ns == 2) { score_rev.assign(n, 0); reversed.assign(n, 0); }
        part_of.assign(n, 0); count.assign(n, 0); first.assign(n, 0);
    }
    // The rows of every finished graph once (k_lg_rows), the jobs' forward passes (and, with pairs, backtracks) in launches that fit
    // the matrix budget, the entries counted, the job table back in one copy, then the entries packed behind the host's prefix
    // offsets and out in one copy.  A job without a forward pass (an empty sequence or graph, the floor of k_lg_prep) never
    // reaches the device; one whose matrix the device cannot hold is VC_WIN_OVERFLOW, and the others run.
    int collect(Run& R, Group& G) override {
        const Kind K = kind(R);
        LArgs a = K.a;
        std::vector<LJob> jobs;
        std::vector<uint32_t> act, refused;                                // jobs with a forward pass; jobs whose matrix the device cannot hold
        uint64_t area = 0;
        for (const uint32_t k : finished(R, G)) {
            const LWin& W = G.hw[k];
            const uint32_t w = G.ids[k];
            const LGraph& g = W.gr[W.cur];
            const uint32_t N = g.n_nodes;
            for (uint32_t s = K.src->win_seq_off[w]; s < K.src->win_seq_off[w + 1]; ++s) {
                LJob J{};
                J.win = k; J.qs = s; J.qlen = (uint32_t)(K.src->seq_off[s + 1] - K.src->seq_off[s]); J.status = VC_WIN_OK;
                if (N != 0 && J.qlen != 0) {                               // else an empty alignment, score 0
                    // the floor of k_lg_prep, and its check of the topological order
                    if (worst_case(a.match, a.gap, a.gap_e, a.gap_q, a.gap_c, (int64_t)J.qlen + 8, N) < (int64_t)KNEG || g.n_rank != N) {
                        J.status = VC_WIN_INVALID;
                    } else {
                        J.rows = N; J.area = area;
                        if (K.pairs) area += (uint64_t)N + J.qlen;
                        act.push_back((uint32_t)jobs.size());
                    }
                }
                jobs.push_back(J);
            }
        }
        if (jobs.empty()) return VC_OK;
        n_jobs += jobs.size();
        std::vector<T> packed;
        if (!act.empty()) {
            DevMem mem;
            LJob* d_job = nullptr; uint32_t* d_list = nullptr; uint64_t* d_hoff = nullptr; int32_t* d_pairs = nullptr; T* d_out = nullptr;
            if (!mem.alloc(&d_job, jobs.size(), jobs.data()) || !mem.alloc(&d_list, act.size()) || !mem.alloc(&d_hoff, act.size()) ||
                (K.pairs && !mem.alloc(&d_pairs, 2 * area)))
                return fail(VC_ERR_HIP, K.no_jobs);
            a.job = d_job; a.q_pairs = d_pairs;
            const uint32_t n = (uint32_t)G.ids.size(), nj = (uint32_t)jobs.size();
            hipLaunchKernelGGL(k_lg_rows, dim3((n + 63) / 64), dim3(64), 0, 0, a);
            if (hipGetLastError() != hipSuccess) return fail(VC_ERR_HIP, K.no_rows);
            auto matrix_cells = [&](uint32_t j) { return ((uint64_t)jobs[j].rows + 1) * ((uint64_t)jobs[j].qlen + 1) * R.planes * K.ns; };
            auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>&, uint64_t, void* H) -> int {
                const uint32_t nl = (uint32_t)list.size();
                f.H = (int32_t*)H;
                with_gap_model(f.gaps, [&](auto gm) { launch_query<decltype(gm)::value>(f, nl, K.ns, K.pairs); });
                if (!ran()) return fail(VC_ERR_HIP, K.no_kernel);
                for (const uint32_t j : list) n_cells += (uint64_t)jobs[j].rows * jobs[j].qlen * K.ns;
                return VC_OK;
            };
            if (const int rc = launch_loop(a, act, R.mat_budget / 4, 4, d_list, d_hoff, K.launch, launches, matrix_cells, as_packed,
                                           [&](uint32_t j) { refused.push_back(j); return VC_OK; }, body))
                return rc;
            if (K.count) {
                K.count(a, nj);
                if (hipGetLastError() != hipSuccess) return fail(VC_ERR_HIP, K.no_count);
            }
            if (hipMemcpy(jobs.data(), d_job, jobs.size() * sizeof(LJob), hipMemcpyDeviceToHost) != hipSuccess) return fail(VC_ERR_HIP, K.no_count);
            bytes += jobs.size() * sizeof(LJob);
            uint64_t total = 0;
            for (LJob& J : jobs) { J.pair_off = total; total += J.*K.n; }
            if (total) {
                packed.resize(NP * total);
                bool ok = mem.alloc(&d_out, NP * total) && hipMemcpy(d_job, jobs.data(), jobs.size() * sizeof(LJob), hipMemcpyHostToDevice) == hipSuccess;
                if (ok) {
                    K.pack(a, d_out, nj, total);
                    ok = hipGetLastError() == hipSuccess && hipMemcpy(packed.data(), d_out, NP * total * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
                }
                if (!ok) return fail(VC_ERR_HIP, K.no_pack);
                bytes += NP * total * sizeof(T);
            }
        }
        for (const uint32_t j : refused) jobs[j].status = VC_WIN_OVERFLOW;
        const uint32_t pi = (uint32_t)part.size();
        for (const LJob& J : jobs) {
            const bool ok = J.status == VC_WIN_OK;
            status[J.qs] = (uint8_t)J.status;
            score[J.qs] = ok ? J.score[0] : 0;
            if (K.ns == 2) { score_rev[J.qs] = ok ? J.score[1] : 0; reversed[J.qs] = ok && J.score[0] < J.score[1]; }
            part_of[J.qs] = pi; first[J.qs] = J.pair_off; count[J.qs] = ok ? J.*K.n : 0;
        }
        part.push_back(std::move(packed));
        return VC_OK;
    }
    // the sequences in batch order (a group that was not computed passes its status on)
    void assemble(const Run& R) override {
        const Kind K = kind(R);
        if (K.pairs) off.assign(K.src->win_seq_off[R.nw] + 1, 0);
        for (uint32_t w = 0; w < R.nw; ++w) {
            for (uint32_t s = K.src->win_seq_off[w]; s < K.src->win_seq_off[w + 1]; ++s) {
                if (R.status[w] != VC_WIN_OK) {
                    status[s] = R.status[w]; score[s] = 0; count[s] = 0;
                    if (!score_rev.empty()) { score_rev[s] = 0; reversed[s] = 0; }
                }
                if (!K.pairs) continue;
                if (count[s]) {
                    const std::vector<T>& p = part[part_of[s]];
                    for (uint32_t x = 0; x < NP; ++x) {
                        const T* src = p.data() + x * (p.size() / NP) + first[s];
                        plane[x].insert(plane[x].end(), src, src + count[s]);
                    }
                }
                off[s + 1] = plane[0].size();
            }
        }
        part.clear();
        if (R.kn.log) std::fprintf(stderr, K.log, (unsigned long long)n_jobs, (unsigned long long)launches, (unsigned long long)n_cells, (unsigned long long)bytes);
    }
};

// vc_poa_run_align (spoa's engine->Align(sequence, graph, &score) for sequences that are NOT added): a job per query of the
// group, the call's engine and the align flags' strands and pairs; the planes are pair_node and pair_pos (k_lg_qpack).
struct AlignStage : JobStage<int32_t, 2> {
    Kind kind(const Run& R) const override {
        return {R.a, R.q.queries, R.q.query_strands(), R.q.query_pairs(), &LJob::npairs, nullptr,
                [](LArgs a, int32_t* d_out, uint32_t nj, uint64_t total) {
                    a.q_out = d_out;
                    hipLaunchKernelGGL(k_lg_qpack, dim3(nj), dim3(64), 0, 0, a, total);
                },
                "device allocation of the query jobs failed", "the query stage's row kernel failed", "a query kernel failed",
                {"device allocation of the query matrices failed", "copy of a query launch failed"},
                "copy of the query jobs failed", "the pack kernel of the query stage or its copy failed",
                "vc_large: align jobs=%llu launches=%llu cells=%llu bytes=%llu\n"};
    }
    void publish(const PoaRequest& q, const vc_batch*) override {
        vc_poa_align_out* ao = q.align;
        if (!ao) return;
        ao->n_queries = q.nq;
        if (!q.has_queries() && q.query_pairs()) off.assign(1, 0);         // no stage ran: the empty tables
        ao->status = table(status); ao->score = table(score);
        if (q.query_strands() == 2) { ao->score_rev = table(score_rev); ao->reversed = table(reversed); }
        if (q.query_pairs()) { ao->pair_off = off.data(); ao->pair_node = table(plane[0]); ao->pair_pos = table(plane[1]); }
        ao->bytes = bytes;
    }
};

// vc_poa_run_correct (GenerateCorrectedSequence of a final local alignment): a job per member of the group, so the "query batch"
// is the group batch itself; kSW with the call's scores and gap model, one strand, always pairs; the pairs with a node are
// counted (k_lg_correct<0>) and the one plane is their nodes' bytes (k_lg_correct<1>, which writes to msa_out).
struct CorrectStage : JobStage<uint8_t, 1> {
    Kind kind(const Run& R) const override {
        LArgs a = R.a;
        a.algorithm = 0;
        a.q_off = a.seq_off; a.q_bases = a.bases; a.q_rc = nullptr;
        return {a, R.b, 1, true, &LJob::ncorr,
                [](const LArgs& a, uint32_t nj) { hipLaunchKernelGGL(k_lg_correct<0>, dim3(nj), dim3(64), 0, 0, a); },
                [](LArgs a, uint8_t* d_out, uint32_t nj, uint64_t) {
                    a.msa_out = d_out;
                    hipLaunchKernelGGL(k_lg_correct<1>, dim3(nj), dim3(64), 0, 0, a);
                },
                "device allocation of the correction jobs failed", "the correction stage's row kernel failed", "a correction kernel failed",
                {"device allocation of the correction matrices failed", "copy of a correction launch failed"},
                "the count kernel of the correction stage or the copy of its jobs failed", "the correction kernel or its copy failed",
                "vc_large: correct jobs=%llu launches=%llu cells=%llu bytes=%llu\n"};
    }
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_correct_out* co = q.correct;
        if (!co) return;
        const uint64_t nseq = b->n_windows ? b->win_seq_off[b->n_windows] : 0;
        if (off.empty()) off.assign(nseq + 1, 0);                          // no run: the empty tables
        co->n_seqs = nseq;
        co->status = table(status); co->score = table(score); co->corr_off = off.data(); co->corr = table(plane[0]);
        co->bytes = bytes;
    }
};

// vc_poa_run_assign: every query of the call against every group, for the best and the second group of each query.  No matrix is
// kept -- a score needs a row only while a successor still reads it --, so a pair costs its group's ring, n_slots x (len + 1)
// cells per plane and strand (k_lg_slots, k_lg_sfwd), and the pairs of a batch of resident groups fill few launches.  The pairs
// are numbered query-major over the batch's finished groups and go through a job table of at most kChunk entries at a time:
// built on the host, uploaded, run in launches that fit the matrix budget, folded on the device (k_lg_assign) and never copied
// back.  What comes back is per query, once per call, and with VC_POA_ASSIGN_SCORES the dense table.
struct AssignStage : Stage {
    static constexpr uint64_t kChunk = 1ull << 16;     // pairs per job table
    std::vector<uint8_t> status, reversed, pair_status;
    std::vector<int32_t> best_g, best_s, sec_g, sec_s, scores;
    uint64_t bytes = 0;                                // copied out of the device
    // until assemble(): the running results on the device, and the job table with its launch lists
    struct Dev {
        DevMem mem;
        LAssign s{};
        LJob* job = nullptr; uint32_t* list = nullptr; uint64_t* hoff = nullptr;
    };
    std::shared_ptr<Dev> dev;
    uint64_t nq = 0, n_pairs = 0, launches = 0, ring_cells = 0, full_cells = 0;
    uint32_t ng = 0, slots_max = 0;

    void size(const Run& R) override { nq = R.q.nq; ng = R.nw; }
    int make_device(const Run& R) {
        static const char* const msg = "device allocation of the assignment tables failed";
        dev = std::make_shared<Dev>();
        Dev& D = *dev;
        LAssign& s = D.s;
        const uint64_t cells = R.q.assign_scores() ? nq * ng : 0;
        if (!D.mem.alloc(&s.best_g, nq) || !D.mem.alloc(&s.best_s, nq) || !D.mem.alloc(&s.sec_g, nq) || !D.mem.alloc(&s.sec_s, nq) ||
            !D.mem.alloc(&s.rev, nq) || !D.mem.alloc(&s.flag, nq) || (cells && (!D.mem.alloc(&s.scores, cells) || !D.mem.alloc(&s.pair_status, cells))) ||
            !D.mem.alloc(&D.job, kChunk) || !D.mem.alloc(&D.list, kChunk) || !D.mem.alloc(&D.hoff, kChunk))
            return fail(VC_ERR_HIP, msg);
        bool ok = hipMemset(s.best_g, 0xFF, nq * 4) == hipSuccess && hipMemset(s.sec_g, 0xFF, nq * 4) == hipSuccess &&
                  hipMemset(s.best_s, 0, nq * 4) == hipSuccess && hipMemset(s.sec_s, 0, nq * 4) == hipSuccess &&
                  hipMemset(s.rev, 0, nq) == hipSuccess && hipMemset(s.flag, 0, nq) == hipSuccess;
        if (cells) ok = ok && hipMemset(s.scores, 0, cells * 4) == hipSuccess && hipMemset(s.pair_status, 0, cells) == hipSuccess;
        s.ng = ng; s.strands = R.q.query_strands();
        return ok ? VC_OK : fail(VC_ERR_HIP, msg);
    }
    int collect(Run& R, Group& G) override {
        static const char* const failed = "an assignment kernel failed";
        const std::vector<uint32_t> fin = finished(R, G);
        if (fin.empty()) return VC_OK;
        if (!dev) if (const int rc = make_device(R)) return rc;
        Dev& D = *dev;
        LArgs a = R.a;
        const uint32_t n = (uint32_t)G.ids.size(), ns = R.q.query_strands();
        // the rows and the slots of every finished graph, once; n_slots back with the windows
        uint32_t* d_gid = nullptr;
        DevMem mem;
        if (!mem.alloc(&d_gid, n, G.ids.data())) return fail(VC_ERR_HIP, "device allocation of the assignment tables failed");
        hipLaunchKernelGGL(k_lg_rows, dim3((n + 63) / 64), dim3(64), 0, 0, a);
        hipLaunchKernelGGL(k_lg_slots, dim3((n + 63) / 64), dim3(64), 0, 0, a);
        if (hipGetLastError() != hipSuccess || hipMemcpy(G.hw.data(), G.d_win, n * sizeof(LWin), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VC_ERR_HIP, "the assignment stage's row or slot kernel failed");
        for (const uint32_t k : fin) if (G.hw[k].gr[G.hw[k].cur].n_nodes) slots_max = std::max(slots_max, G.hw[k].n_slots);
        a.job = D.job;
        LAssign s = D.s;
        s.gid = d_gid; s.nfin = (uint32_t)fin.size();
        const uint64_t T = nq * fin.size();
        std::vector<LJob> jobs;
        std::vector<uint32_t> act;
        const vc_batch* qb = R.q.queries;
        for (uint64_t t0 = 0; t0 < T; t0 += kChunk) {
            const uint64_t t1 = std::min(T, t0 + kChunk);
            jobs.assign(t1 - t0, LJob{});
            act.clear();
            for (uint64_t t = t0; t < t1; ++t) {
                LJob& J = jobs[t - t0];
                const uint32_t k = fin[t % fin.size()];
                const LGraph& g = G.hw[k].gr[G.hw[k].cur];
                const uint32_t N = g.n_nodes;
                J.win = k; J.qs = (uint32_t)(t / fin.size()); J.qlen = (uint32_t)(qb->seq_off[J.qs + 1] - qb->seq_off[J.qs]); J.status = VC_WIN_OK;
                if (N == 0 || J.qlen == 0) continue;                       // an empty alignment, score 0
                // the floor of k_lg_prep, and its check of the topological order (JobStage::collect)
                if (worst_case(a.match, a.gap, a.gap_e, a.gap_q, a.gap_c, (int64_t)J.qlen + 8, N) < (int64_t)KNEG || g.n_rank != N || G.hw[k].n_slots == 0) {
                    J.status = VC_WIN_INVALID;
                    continue;
                }
                J.rows = N;
                act.push_back((uint32_t)(t - t0));
            }
            if (hipMemcpy(D.job, jobs.data(), jobs.size() * sizeof(LJob), hipMemcpyHostToDevice) != hipSuccess)
                return fail(VC_ERR_HIP, "copy of the assignment jobs failed");
            auto columns = [&](uint32_t j) { return ((uint64_t)jobs[j].qlen + 1) * R.planes * ns; };
            auto ring = [&](uint32_t j) { return (uint64_t)G.hw[jobs[j].win].n_slots * columns(j); };
            auto refuse = [&](uint32_t j) -> int {                         // the device has no room for this one ring
                jobs[j].status = VC_WIN_OVERFLOW;
                return hipMemcpy(D.job + j, &jobs[j], sizeof(LJob), hipMemcpyHostToDevice) == hipSuccess ? VC_OK : fail(VC_ERR_HIP, failed);
            };
            auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>&, uint64_t cells, void* H) -> int {
                f.H = (int32_t*)H;
                with_gap_model(f.gaps, [&](auto gm) { hipLaunchKernelGGL(k_lg_sfwd<decltype(gm)::value>, dim3((uint32_t)list.size(), ns), dim3(64), 0, 0, f); });
                if (hipGetLastError() != hipSuccess) return fail(VC_ERR_HIP, failed);
                ring_cells += cells;
                for (const uint32_t j : list) full_cells += ((uint64_t)jobs[j].rows + 1) * columns(j);
                return VC_OK;
            };
            if (const int rc = launch_loop(a, act, R.mat_budget / 4, 4, D.list, D.hoff,
                                           {"device allocation of the assignment rings failed", "copy of an assignment launch failed"}, launches,
                                           ring, as_packed, refuse, body))
                return rc;
            s.t0 = t0; s.t1 = t1;
            const uint64_t lanes = (t1 - 1) / fin.size() - t0 / fin.size() + 1;
            hipLaunchKernelGGL(k_lg_assign, dim3((uint32_t)((lanes + 63) / 64)), dim3(64), 0, 0, a, s);
            if (!ran()) return fail(VC_ERR_HIP, failed);
            n_pairs += t1 - t0;
        }
        return VC_OK;
    }
    // the per-query results back, once; the groups that were not computed pass their status on to their pairs
    void assemble(const Run& R) override {
        const bool dense = R.q.assign_scores();
        status.assign(nq, VC_WIN_OK); reversed.assign(nq, 0);
        best_g.assign(nq, -1); sec_g.assign(nq, -1); best_s.assign(nq, 0); sec_s.assign(nq, 0);
        if (dense) { scores.assign(nq * ng, 0); pair_status.assign(nq * ng, VC_WIN_OK); }
        std::vector<uint8_t> flag(nq, 0);
        if (dev) {
            const LAssign& s = dev->s;
            bool ok = hipMemcpy(best_g.data(), s.best_g, nq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(best_s.data(), s.best_s, nq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(sec_g.data(), s.sec_g, nq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(sec_s.data(), s.sec_s, nq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(reversed.data(), s.rev, nq, hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(flag.data(), s.flag, nq, hipMemcpyDeviceToHost) == hipSuccess;
            bytes += 18 * nq;
            if (dense && nq * ng) {
                ok = ok && hipMemcpy(scores.data(), s.scores, nq * ng * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                     hipMemcpy(pair_status.data(), s.pair_status, nq * ng, hipMemcpyDeviceToHost) == hipSuccess;
                bytes += 5 * nq * ng;
            }
            copy_failed = !ok;
            dev.reset();
        }
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] == VC_WIN_OK) continue;
            for (uint64_t k = 0; k < nq; ++k) {
                flag[k] |= R.status[w] == VC_WIN_OVERFLOW ? 1 : 2;
                if (dense) { scores[k * ng + w] = 0; pair_status[k * ng + w] = R.status[w]; }
            }
        }
        for (uint64_t k = 0; k < nq; ++k) status[k] = (flag[k] & 1) ? VC_WIN_OVERFLOW : (flag[k] & 2) ? VC_WIN_INVALID : VC_WIN_OK;
        if (R.kn.log)
            std::fprintf(stderr, "vc_large: assign groups=%u queries=%llu pairs=%llu launches=%llu slots_max=%u ring_cells=%llu full_cells=%llu\n", ng,
                         (unsigned long long)nq, (unsigned long long)n_pairs, (unsigned long long)launches, slots_max,
                         (unsigned long long)ring_cells, (unsigned long long)full_cells);
    }
    bool copy_failed = false;                          // assemble() cannot fail: poa_run asks afterwards
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_assign_out* o = q.assign;
        if (!o) return;
        const uint64_t cells = q.nq * b->n_windows;
        if (best_g.size() != q.nq) {                                       // no stage ran (no query, or no group): the "none" values
            status.assign(q.nq, VC_WIN_OK); reversed.assign(q.nq, 0);
            best_g.assign(q.nq, -1); sec_g.assign(q.nq, -1); best_s.assign(q.nq, 0); sec_s.assign(q.nq, 0);
        }
        if (q.assign_scores() && scores.size() != cells) { scores.assign(cells, 0); pair_status.assign(cells, VC_WIN_OK); }
        o->n_queries = q.nq; o->n_groups = b->n_windows;
        o->status = table(status);
        o->best_group = table(best_g); o->best_score = table(best_s); o->second_group = table(sec_g); o->second_score = table(sec_s);
        if (q.query_strands() == 2) o->reversed = table(reversed);
        if (q.assign_scores()) { o->scores = table(scores); o->pair_status = table(pair_status); }
        o->bytes = bytes;
    }
};

// The haplotypes of every group (vc_poa_hap_out): a block and a scratch per group in the matrix buffer, laid out as the graph
// stage's are.  k_lg_hap splits the members; k_lg_hapcons then runs on a grid of (groups, max_haplotypes), one block per
// haplotype that exists, so no count has to come back in between.
struct HapStage : Stage {
    std::vector<uint32_t> n_haps, hap_size, site_col, site_n1, site_n2;
    std::vector<uint64_t> hap_first, cons_off, site_off;
    std::vector<uint8_t> cons, hap_of, site_major, site_minor;
    uint64_t bytes = 0;                                // copied out of the device
    // until assemble(), per window: its block and the counts that lay it out
    struct Part { uint32_t S = 0, C = 0, N = 0; std::vector<uint8_t> blk; };
    std::vector<Part> part;
    uint64_t launches = 0;

    void size(const Run& R) override { part.resize(R.nw); }
    int collect(Run& R, Group& G) override {
        const LArgs& a = R.a;
        const vc_poa_hap_params& h = *R.q.hap;
        const LHap hp{h.max_haplotypes, h.min_reads, h.min_permille, h.rounds, h.flags};
        auto counts_of = [&](uint32_t k) {
            const LWin& W = G.hw[k];
            Part p;
            p.S = W.gr[W.cur].nseq; p.C = W.gr_cols; p.N = W.gr[W.cur].n_nodes;
            return p;
        };
        auto block_of = [&](uint32_t k) { const Part p = counts_of(k); return hap_block(p.S, p.C, p.N, hp.max_haps).bytes; };
        auto scratch_of = [&](uint32_t k) {
            const Part p = counts_of(k);
            return hap_scratch(p.S, p.C, G.hw[k].gr_path, p.N, G.hw[k].gr[G.hw[k].cur].n_edges, hp.max_haps).bytes;
        };
        uint64_t blocks = 0;
        std::vector<uint8_t> host;
        auto body = [&](LArgs& f, const std::vector<uint32_t>& list, const std::vector<uint64_t>& hoff, uint64_t, void* dout) -> int {
            const uint32_t nl = (uint32_t)list.size();
            f.msa_out = (uint8_t*)dout;
            hipLaunchKernelGGL(k_lg_hap, dim3(nl), dim3(64), 0, 0, f, hp);
            hipLaunchKernelGGL(k_lg_hapcons, dim3(nl, hp.max_haps), dim3(64), 0, 0, f, hp);
            auto part_of = [&](uint32_t q) -> std::vector<uint8_t>& {
                Part& p = part[G.ids[list[q]]];
                p = counts_of(list[q]);
                return p.blk;
            };
            if (hipGetLastError() != hipSuccess || !blocks_out(dout, blocks, hoff, nl, host, part_of))
                return fail(VC_ERR_HIP, "a haplotype kernel or its copy failed");
            bytes += blocks;
            return VC_OK;
        };
        return launch_loop(a, finished(R, G), R.mat_budget, 1, G.d_list, G.d_hoff,
                           {"device allocation of the haplotype tables failed", "a haplotype kernel or its copy failed"}, launches,
                           [&](uint32_t k) { return block_of(k) + scratch_of(k); },
                           [&](const std::vector<uint32_t>& list, std::vector<uint64_t>& hoff) { blocks = blocks_first(list, hoff, block_of, scratch_of); },
                           [&](uint32_t k) { return refuse_group(R, G.ids[k]); }, body);
    }
    // the tables in window order; the members from labels to sequences of the batch
    void assemble(const Run& R) override {
        const uint32_t maxh = R.q.hap->max_haplotypes;
        hap_first.assign(1, 0); cons_off.assign(1, 0); site_off.assign(1, 0);
        hap_of.assign(R.nseq_all, VC_POA_HAP_NONE);
        for (uint32_t w = 0; w < R.nw; ++w) {
            if (R.status[w] != VC_WIN_OK) part[w] = Part{};
            const Part& p = part[w];
            uint32_t K = 0;
            if (!p.blk.empty()) {
                const HapBlock B = hap_block(p.S, p.C, p.N, maxh);
                const uint8_t* blk = p.blk.data();
                const uint32_t* head = (const uint32_t*)blk;
                K = head[0];
                const uint32_t M = head[1];
                for (uint32_t k = 0; k < K; ++k) {
                    hap_size.push_back(head[2 + k]);
                    const uint8_t* c = blk + B.cons + (uint64_t)k * p.N;
                    cons.insert(cons.end(), c, c + head[2 + VC_POA_HAP_MAX + k]);
                    cons_off.push_back(cons.size());
                }
                const uint32_t* mem = (const uint32_t*)(blk + B.member);
                for (uint32_t s = 0; s < p.S; ++s) hap_of[R.b->win_seq_off[w] + mem[s]] = blk[B.hap_of + s];
                const uint32_t *col = (const uint32_t*)(blk + B.s_col), *n1 = (const uint32_t*)(blk + B.s_n1), *n2 = (const uint32_t*)(blk + B.s_n2);
                site_col.insert(site_col.end(), col, col + M); site_n1.insert(site_n1.end(), n1, n1 + M); site_n2.insert(site_n2.end(), n2, n2 + M);
                site_major.insert(site_major.end(), blk + B.s_maj, blk + B.s_maj + M);
                site_minor.insert(site_minor.end(), blk + B.s_min, blk + B.s_min + M);
            }
            n_haps.push_back(K);
            hap_first.push_back(hap_size.size());
            site_off.push_back(site_col.size());
            part[w] = Part{};
        }
        if (R.kn.log) std::fprintf(stderr, "vc_large: haplotypes launches=%llu bytes=%llu\n", (unsigned long long)launches, (unsigned long long)bytes);
    }
    void publish(const PoaRequest& q, const vc_batch* b) override {
        vc_poa_hap_out* o = q.haps;
        if (!o) return;
        o->n_groups = b->n_windows;
        if (!b->n_windows) return;
        o->n_haps = table(n_haps); o->hap_first = hap_first.data(); o->hap_size = table(hap_size);
        o->cons_off = cons_off.data(); o->cons = table(cons); o->hap_of = table(hap_of);
        o->site_off = site_off.data(); o->site_col = table(site_col); o->site_major = table(site_major); o->site_minor = table(site_minor);
        o->site_n_major = table(site_n1); o->site_n_minor = table(site_n2);
        o->bytes = bytes;
    }
};

// The stages of the process, and with them what the vc_poa_* entries hand out: valid until the next call that has an output of
// its own (poa_run clears them then, and when such a call fails) or vc_large_release.
struct Outputs {
    MsaStage msa;
    ProfileStage profile;
    GraphStage graph;
    CorrectStage correct;
    AlignStage align;
    AssignStage assign;
    HapStage haps;
    // The stages that run in a call, in the order run_group collects and run_windows assembles them.  Correct stands before
    // align as run_group always had them, align before correct in run_windows: one order serves both, because the two never
    // occur in one call (only vc_poa_run_correct asks for correction, and it takes no query batch).
    std::vector<Stage*> active(const PoaRequest& q) {
        std::vector<Stage*> s;
        if (q.rows()) s.push_back(&msa);
        if (q.profile) s.push_back(&profile);
        if (q.graph) s.push_back(&graph);
        if (q.correct) s.push_back(&correct);
        if (q.has_queries() && q.align) s.push_back(&align);
        if (q.has_queries() && q.assign) s.push_back(&assign);
        if (q.haps) s.push_back(&haps);
        return s;
    }
    std::vector<Stage*> all() { return {&msa, &profile, &graph, &correct, &align, &assign, &haps}; }
    void clear() { *this = Outputs{}; }
} g_out;

// One group from its tables to its results: a window whose table filled goes back to pending, the others leave their status,
// consensus and outputs.  A single window the device has no room for is VC_WIN_OVERFLOW; more than one is an error.
int run_group(Run& R, Group& G) {
    const uint32_t n = (uint32_t)G.ids.size();
    uint8_t* arena = (uint8_t*)cached(g_cache.arena, G.abytes);
    DevMem mem;
    if (!arena || !mem.alloc(&G.d_win, n) || !mem.alloc(&G.d_list, n) || !mem.alloc(&G.d_hoff, R.q.graph || R.q.profile || R.q.haps ? 2 * (size_t)n : n)) {
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
        R.out[w].resize(R.a.correct && W.status != VC_WIN_OK ? 0 : W.cons_n);          // (a group that failed in a round keeps no consensus)
        if (!R.out[w].empty() && hipMemcpy(R.out[w].data(), W.cons, W.cons_n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VC_ERR_HIP, "copy of a consensus failed");
    }
    for (Stage* s : R.stages) if (const int rc = s->collect(R, G)) return rc;
    return VC_OK;
}

// vc_poa_run_strand: the choices; zeros for the groups that were not computed
int copy_strands(const Run& R) {
    const vc_batch* b = R.b;
    const vc_poa_strand_out* so = R.q.strand;
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

// the closing log line, then consensus and status in window order
int assemble(Run& R, vc_result* r) {
    if (R.kn.log && R.a.spans) {
        Run::SpanCount t;
        for (const Run::SpanCount& c : R.sp_of) { t.members += c.members; t.rows += c.rows; t.full += c.full; }
        std::fprintf(stderr, "vc_large: spans members=%llu sub_rows=%llu full_rows=%llu\n", (unsigned long long)t.members,
                     (unsigned long long)t.rows, (unsigned long long)t.full);
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

// the run after every argument check (mode 0 / 1: the windows carry spans; mode 1 reads edge labels); g_out is clear where q asks for an output
int run_windows(int32_t device, const LArgs& a, const vc_batch* b, std::vector<Caps>& caps, const Knobs& kn, vc_result* r, const PoaRequest& q) {
    const uint32_t nw = b->n_windows;
    if (hipSetDevice(device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");
    if (g_cache.device != device) { release_cache(); g_cache.device = device; }
    Run R{a, b, caps, kn, q, a.mode == 1 || q.keeps_labels(), nw, b->win_seq_off[nw], b->seq_off[b->win_seq_off[nw]]};
    DevMem mem;                                                            // the batch and the strand views: held until the call ends
    if (const int rc = upload_batch(R, mem, a.mode != 2)) return rc;
    if (q.spans) {                                                         // vc_poa_run_spans: the spans where the windows' positions go
        uint32_t *d_sb = nullptr, *d_se = nullptr;
        if (!mem.alloc(&d_sb, R.nseq_all, q.spans->begin) || !mem.alloc(&d_se, R.nseq_all, q.spans->end))
            return fail(VC_ERR_HIP, "device allocation or copy of the spans failed");
        R.a.seq_begin = d_sb; R.a.seq_end = d_se; R.a.spans = 1;
        R.sp_of.resize(nw);
    }
    if (q.weights) {                                                       // vc_poa_run_weighted with a weighted member: k_lg_apply<true> reads these
        uint8_t* d_m = nullptr; uint32_t *d_sw = nullptr, *d_bw = nullptr;
        if (!mem.alloc(&d_m, R.nseq_all, q.weights->mode) || !mem.alloc(&d_sw, R.nseq_all, q.weights->seq_weight) ||
            (q.base_weights && !mem.alloc(&d_bw, R.nbytes, q.weights->base_weight)))
            return fail(VC_ERR_HIP, "device allocation or copy of the weights failed");
        R.a.wmode = d_m; R.a.seq_w = d_sw; R.a.base_w = d_bw;
    }
    if (q.strand) if (const int rc = strand_views(R, mem)) return rc;
    if (q.from) if (const int rc = upload_stored(R, mem)) return rc;
    if (q.has_queries()) if (const int rc = upload_queries(R, mem)) return rc;

    // budgets from free device memory (what this library keeps cached counts as free)
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint64_t avail = free_b + g_cache.arena.bytes + g_cache.mat.bytes;
    R.arena_budget = kn.arena ? kn.arena : std::min<uint64_t>(avail / 4, 16ull << 30);
    R.mat_budget = kn.mat ? kn.mat : std::min<uint64_t>(avail / 2, 48ull << 30);
    R.planes = plane_count(a.gaps);
    R.ns = q.strands();

    R.out.resize(nw);
    R.status.assign(nw, VC_WIN_OVERFLOW);
    R.stages = g_out.active(q);
    for (Stage* s : R.stages) s->size(R);
    R.pending.resize(nw);
    for (uint32_t w = 0; w < nw; ++w) R.pending[w] = w;
    while (!R.pending.empty()) {
        Group G;
        next_group(R, G);
        if (G.ids.empty()) continue;
        if (const int rc = run_group(R, G)) return rc;
    }
    if (q.strand) if (const int rc = copy_strands(R)) return rc;
    for (Stage* s : R.stages) s->assemble(R);
    if (g_out.assign.copy_failed) return fail(VC_ERR_HIP, "copy of the assignment results failed");
    return assemble(R, r);
}

// vc_poa_run_align's own arguments, after the batch and before the device: the output and its flags, the query batch and its
// count against the groups, the query lengths.  vc_poa_run_assign shares the query batch's checks: its windows mean nothing
// (their last offset is the sequence count), its output was checked at the entry and its flags come after `from`.
int check_queries(PoaRequest& A, const vc_batch* b) {
    if (!A.assign && !A.align) return fail(VC_ERR_ARG, "null align output");
    if (A.align_flags & ~(uint32_t)(VC_POA_ALIGN_PAIRS | VC_POA_ALIGN_STRANDS)) return fail(VC_ERR_ARG, "unknown align flag bits");
    const vc_batch* q = A.queries;
    if (!q) return fail(VC_ERR_ARG, "null query batch");
    if (!A.assign && q->n_windows != b->n_windows) return fail(VC_ERR_ARG, "the query batch needs one window per group");
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

// The counts of stored graph w of a vc_poa_graph_in that check_from has passed: nodes, edges, aligned-list cells, paths, path entries
struct StoredCounts { uint64_t N, E, A, S, T; };
StoredCounts stored_counts(const vc_poa_graph_in* f, uint32_t w) {
    const uint64_t N = f->n_nodes[w], ob = f->node_off[w] + w, p0 = f->path_first[w], S = f->path_first[w + 1] - p0;
    return {N, f->out_off[ob + N] - f->out_off[ob], f->al_off[ob + N] - f->al_off[ob], S, f->path_off[p0 + S] - f->path_off[p0]};
}

// vc_poa_run_from's stored graphs, after the batch and the queries and before the device.  They are untrusted: the kernels index
// with what they hold, so every rule is checked here, in the order the header states: the arrays and the group count; the
// offsets; the node ids; the topological order; the aligned lists; the paths; the member numbers.
int check_from(const vc_poa_graph_in* f, const vc_batch* b) {
    const uint32_t ng = f->n_groups;
    if (ng != b->n_windows) return fail(VC_ERR_ARG, "the stored graphs need one graph per group");
    if (ng == 0) return VC_OK;
    if (!f->n_members || !f->n_nodes || !f->node_off || !f->out_off || !f->al_off || !f->path_first || !f->path_off)
        return fail(VC_ERR_ARG, "null array in the stored graphs");
    // offsets: prefix sums that start at 0 and never decrease; a path has a node; every count of a group stays below 2^31
    if (f->node_off[0] != 0 || f->path_first[0] != 0 || f->path_off[0] != 0 || f->out_off[0] != 0 || f->al_off[0] != 0)
        return fail(VC_ERR_ARG, "an offset table of the stored graphs does not start at 0");
    constexpr uint64_t kMax = 1ull << 31;
    for (uint32_t w = 0; w < ng; ++w) {
        if (f->n_nodes[w] >= kMax || f->node_off[w + 1] < f->node_off[w] || f->node_off[w + 1] - f->node_off[w] != f->n_nodes[w])
            return fail(VC_ERR_ARG, "node_off of the stored graphs is not the prefix sum of n_nodes");
        if (f->path_first[w + 1] < f->path_first[w] || f->path_first[w + 1] - f->path_first[w] >= kMax)
            return fail(VC_ERR_ARG, "path_first of the stored graphs decreases");
    }
    const uint64_t NN = f->node_off[ng], PP = f->path_first[ng];
    for (uint64_t k = 1; k < NN + ng; ++k)
        if (f->out_off[k] < f->out_off[k - 1] || f->al_off[k] < f->al_off[k - 1]) return fail(VC_ERR_ARG, "out_off or al_off of the stored graphs decreases");
    for (uint64_t k = 0; k < PP; ++k)
        if (f->path_off[k + 1] <= f->path_off[k]) return fail(VC_ERR_ARG, "path_off of the stored graphs does not increase (a path has at least one node)");
    const uint64_t EE = f->out_off[NN + ng - 1], AA = f->al_off[NN + ng - 1], TT = f->path_off[PP];
    for (uint32_t w = 0; w < ng; ++w) {
        const StoredCounts c = stored_counts(f, w);
        if (c.E >= kMax || c.A >= kMax || c.T >= kMax) return fail(VC_ERR_ARG, "a stored graph is too large (2^31 edges, aligned cells or path entries)");
    }
    if ((NN && (!f->node_base || !f->rank_to_node)) || (EE && (!f->edge_head || !f->edge_weight)) || (AA && !f->al_node) ||
        (PP && (!f->path_member || !f->path_reversed)) || (TT && !f->path_node))
        return fail(VC_ERR_ARG, "null array in the stored graphs");
    // node ids
    for (uint32_t w = 0; w < ng; ++w) {
        const uint64_t N = f->n_nodes[w], nb = f->node_off[w], ob = nb + w, p0 = f->path_first[w], p1 = f->path_first[w + 1];
        for (uint64_t k = f->out_off[ob]; k < f->out_off[ob + N]; ++k) if (f->edge_head[k] >= N) return fail(VC_ERR_ARG, "edge_head of the stored graphs names no node");
        for (uint64_t k = f->al_off[ob]; k < f->al_off[ob + N]; ++k) if (f->al_node[k] >= N) return fail(VC_ERR_ARG, "al_node of the stored graphs names no node");
        for (uint64_t k = f->path_off[p0]; k < f->path_off[p1]; ++k) if (f->path_node[k] >= N) return fail(VC_ERR_ARG, "path_node of the stored graphs names no node");
        for (uint64_t v = 0; v < N; ++v) if (f->rank_to_node[nb + v] >= N) return fail(VC_ERR_ARG, "rank_to_node of the stored graphs names no node");
    }
    // the topological order: a permutation in which every edge runs forward
    std::vector<uint32_t> rank_of;
    for (uint32_t w = 0; w < ng; ++w) {
        const uint64_t N = f->n_nodes[w], nb = f->node_off[w], ob = nb + w;
        rank_of.assign(N, NONE);
        for (uint64_t r = 0; r < N; ++r) {
            uint32_t& x = rank_of[f->rank_to_node[nb + r]];
            if (x != NONE) return fail(VC_ERR_ARG, "rank_to_node of the stored graphs is not a permutation");
            x = (uint32_t)r;
        }
        for (uint64_t v = 0; v < N; ++v)
            for (uint64_t k = f->out_off[ob + v]; k < f->out_off[ob + v + 1]; ++k)
                if (rank_of[f->edge_head[k]] <= rank_of[v]) return fail(VC_ERR_ARG, "an edge of the stored graphs runs against rank_to_node");
    }
    // aligned lists: not the node itself, no node twice, and symmetric
    for (uint32_t w = 0; w < ng; ++w) {
        const uint64_t N = f->n_nodes[w], ob = f->node_off[w] + w;
        for (uint64_t v = 0; v < N; ++v) {
            const uint64_t a0 = f->al_off[ob + v], a1 = f->al_off[ob + v + 1];
            for (uint64_t k = a0; k < a1; ++k) {
                if (f->al_node[k] == v) return fail(VC_ERR_ARG, "an aligned list of the stored graphs holds its own node");
                for (uint64_t j = a0; j < k; ++j) if (f->al_node[j] == f->al_node[k]) return fail(VC_ERR_ARG, "an aligned list of the stored graphs holds a node twice");
            }
            for (uint64_t k = a0; k < a1; ++k) {
                const uint32_t u = f->al_node[k];
                bool back = false;
                for (uint64_t j = f->al_off[ob + u]; j < f->al_off[ob + u + 1] && !back; ++j) back = f->al_node[j] == v;
                if (!back) return fail(VC_ERR_ARG, "the aligned lists of the stored graphs are not symmetric");
            }
        }
    }
    // ... and never joined by an edge (they share a column of the alignment)
    for (uint32_t w = 0; w < ng; ++w) {
        const uint64_t N = f->n_nodes[w], ob = f->node_off[w] + w;
        for (uint64_t v = 0; v < N; ++v)
            for (uint64_t k = f->out_off[ob + v]; k < f->out_off[ob + v + 1]; ++k)
                for (uint64_t j = f->al_off[ob + v]; j < f->al_off[ob + v + 1]; ++j)
                    if (f->al_node[j] == f->edge_head[k]) return fail(VC_ERR_ARG, "aligned nodes of the stored graphs are joined by an edge");
    }
    // paths: every consecutive pair is an edge of the tail's out-list (the first with that head, as add_edge finds it), and every
    // edge lies on a path: an edge no sequence walked would be in no in-list (a second edge u -> v never is walked)
    std::vector<uint8_t> walked;
    for (uint32_t w = 0; w < ng; ++w) {
        const uint64_t N = f->n_nodes[w], ob = f->node_off[w] + w, e0 = f->out_off[ob];
        walked.assign(f->out_off[ob + N] - e0, 0);
        for (uint64_t p = f->path_first[w]; p < f->path_first[w + 1]; ++p) {
            for (uint64_t k = f->path_off[p]; k + 1 < f->path_off[p + 1]; ++k) {
                const uint32_t u = f->path_node[k], v = f->path_node[k + 1];
                bool edge = false;
                for (uint64_t j = f->out_off[ob + u]; j < f->out_off[ob + u + 1] && !edge; ++j)
                    if ((edge = f->edge_head[j] == v)) walked[j - e0] = 1;
                if (!edge) return fail(VC_ERR_ARG, "a path of the stored graphs steps along no edge");
            }
        }
        for (const uint8_t x : walked) if (!x) return fail(VC_ERR_ARG, "an edge of the stored graphs lies on no path");
    }
    // member numbers; the members to come must still fit 32 bits
    for (uint32_t w = 0; w < ng; ++w) {
        for (uint64_t p = f->path_first[w]; p < f->path_first[w + 1]; ++p)
            if (f->path_member[p] >= f->n_members[w]) return fail(VC_ERR_ARG, "path_member of the stored graphs is not below n_members");
        if ((uint64_t)f->n_members[w] + (b->win_seq_off[w + 1] - b->win_seq_off[w]) >= VC_POA_ROW_CONSENSUS)
            return fail(VC_ERR_ARG, "n_members of the stored graphs leaves no room for the new members");
    }
    return VC_OK;
}

// vc_poa_run_spans' spans, after the batch and before the device.  They are untrusted and become node ids on the device, so
// every rule is checked here, member by member in batch order: both entries NONE or neither; begin <= end; end on sequence 0 of
// the group (whose base k is node k: the group is built from nothing).  Sequence 0's own entries are not read.  A call in which
// no member has a span is the call without spans: A.spans is cleared and nothing of them reaches the device.
int check_spans(PoaRequest& A, const vc_batch* b) {
    const vc_poa_span_in* sp = A.spans;
    A.spans = nullptr;
    const uint32_t nw = b->n_windows;
    if (!sp || nw == 0 || b->win_seq_off[nw] == 0) return VC_OK;
    if (!sp->begin || !sp->end) return fail(VC_ERR_ARG, "null span array");
    bool any = false;
    char msg[160];
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t s0 = b->win_seq_off[w], s1 = b->win_seq_off[w + 1];
        for (uint32_t s = s0 + 1; s < s1; ++s) {
            const uint32_t sb = sp->begin[s], se = sp->end[s];
            if (sb == VC_POA_SPAN_NONE && se == VC_POA_SPAN_NONE) continue;
            const uint64_t L = b->seq_off[s0 + 1] - b->seq_off[s0];
            const char* what = sb == VC_POA_SPAN_NONE || se == VC_POA_SPAN_NONE ? "has only one of begin and end set to VC_POA_SPAN_NONE"
                               : sb > se                                       ? "begins behind its end"
                               : se >= L                                       ? "ends beyond sequence 0 of its group"
                                                                               : nullptr;
            if (what) {
                std::snprintf(msg, sizeof msg, "the span of member %u of group %u %s", s - s0, w, what);
                return fail(VC_ERR_ARG, msg);
            }
            any = true;
        }
    }
    if (any) A.spans = sp;
    return VC_OK;
}

// vc_poa_run_weighted's weights, after the batch and before the device, in the header's order, one kind of violation after the
// other and each member by member in batch order: the mode array NULL; a mode above 2; seq_weight NULL beside a mode-1 member;
// base_weight NULL beside a mode-2 member.  A call in which every member has mode 0 is the call without weights: A.weights is
// cleared and nothing of them reaches the device.
int check_weights(PoaRequest& A, const vc_batch* b) {
    const vc_poa_weight_in* wt = A.weights;
    A.weights = nullptr; A.base_weights = false;
    if (!wt) return VC_OK;
    if (!wt->mode) return fail(VC_ERR_ARG, "null weight mode array");
    const uint32_t nw = b->n_windows;
    // the first member the rule `bad` names, as the message says it
    auto first = [&](auto bad, const char* what) -> int {
        for (uint32_t w = 0; w < nw; ++w)
            for (uint32_t s0 = b->win_seq_off[w], s = s0; s < b->win_seq_off[w + 1]; ++s)
                if (bad(wt->mode[s])) {
                    char msg[160];
                    std::snprintf(msg, sizeof msg, "the weight mode of member %u of group %u %s", s - s0, w, what);
                    return fail(VC_ERR_ARG, msg);
                }
        return VC_OK;
    };
    if (const int rc = first([](uint8_t m) { return m > 2; }, "is not 0, 1 or 2")) return rc;
    if (!wt->seq_weight) if (const int rc = first([](uint8_t m) { return m == 1; }, "is 1 beside a null seq_weight")) return rc;
    if (!wt->base_weight) if (const int rc = first([](uint8_t m) { return m == 2; }, "is 2 beside a null base_weight")) return rc;
    bool any = false;
    for (uint32_t s = 0, n = nw ? b->win_seq_off[nw] : 0; s < n; ++s) { any |= wt->mode[s] != 0; A.base_weights |= wt->mode[s] == 2; }
    if (any) A.weights = wt;
    return VC_OK;
}

// The vc_poa_* entries after their score checks: the knobs, the batch (still without the device), the queries, the device, the
// run.  `a` holds the scores.
int run_groups(int32_t device, int32_t algorithm, LArgs a, const vc_batch* b, vc_result* r, PoaRequest& q) {
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
    if (q.required & (PoaRequest::ALIGN | PoaRequest::ASSIGN)) if (const int rc = check_queries(q, b)) return rc;
    if (q.from) {
        if (const int rc = check_from(q.from, b)) return rc;
        // tables: the stored counts, and beside them the usual allowance for the new members (which alone the knobs shrink)
        for (uint32_t w = 0; w < nw; ++w) {
            const StoredCounts c = stored_counts(q.from, w);
            Caps& k = caps[w];
            k.NC += c.N; k.EC += c.E; k.AC += c.A; k.LC += c.T; k.SC += c.N + c.E + c.A; k.PC += c.N; k.nseq += c.S;
        }
    }
    if (q.assign_flags & ~(uint32_t)(VC_POA_ASSIGN_STRANDS | VC_POA_ASSIGN_SCORES)) return fail(VC_ERR_ARG, "unknown assign flag bits");
    if (const int rc = check_spans(q, b)) return rc;
    if (const int rc = check_weights(q, b)) return rc;
    a.num_prune = 1;
    if (q.required & PoaRequest::CORRECT) {
        // vc_poa_run_correct's own arguments, after the batch and before the device
        if (q.prune->num_prune == 0) return fail(VC_ERR_ARG, "num_prune must be >= 1 (the reference's num_prune - 1 rounds would wrap)");
        if (!(q.prune->min_confidence >= 0) || !(q.prune->min_support >= 0)) return fail(VC_ERR_ARG, "min_confidence and min_support must be >= 0 and not NaN");
        a.correct = 1; a.min_conf = q.prune->min_confidence; a.min_sup = q.prune->min_support; a.num_prune = q.prune->num_prune;
    }
    if (const int rc = check_device(device, "the large-graph path", g_err)) return rc;
    r->cons_off[0] = 0;
    if (nw == 0) return VC_OK;
    a.mode = 2; a.algorithm = (uint32_t)algorithm;
    return run_windows(device, a, b, caps, kn, r, q);
}

// Every vc_poa_* entry behind its request (vc_poa_run after its own checks).  The arguments first, without the device, in
// AlignmentEngine::Create's order (alignment_engine.cpp:39-57; spoa takes the scores as int8_t); then the flags, the graph output,
// the strand output; the batch and the queries in run_groups.  Then the run, and g_out's parts published into their out-structs.
int poa_run(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, PoaRequest q) {
    vc_poa_msa_out* const o = q.msa;
    if (q.graph) *q.graph = vc_poa_graph_out{};                            // a failed call leaves every pointer NULL
    if (q.align) { q.align_flags = q.align->flags; *q.align = vc_poa_align_out{}; q.align->flags = q.align_flags; }
    if (q.correct) *q.correct = vc_poa_correct_out{};
    if (q.state) *q.state = vc_poa_state_out{};
    if (q.profile) *q.profile = vc_poa_profile_out{};
    if (q.assign) { q.assign_flags = q.assign->flags; *q.assign = vc_poa_assign_out{}; q.assign->flags = q.assign_flags; }
    if (q.haps) *q.haps = vc_poa_hap_out{};
    if (!p || !b || !r || ((q.required & PoaRequest::HAPS) && (!q.hap || !q.haps)) || ((q.required & PoaRequest::MSA) && !o) || ((q.required & PoaRequest::CORRECT) && (!q.prune || !q.correct)) || !r->cons_off || !r->status || (!r->cons && r->cons_cap)) return fail(VC_ERR_ARG, "null argument");
    if (p->algorithm < 0 || p->algorithm > 2) return fail(VC_ERR_ARG, "algorithm must be 0 (local), 1 (global) or 2 (semi-global)");
    if (p->gap_open > 0 || p->gap_open2 > 0) return fail(VC_ERR_ARG, "gap opening penalties must be <= 0");
    if (p->gap_extend > 0 || p->gap_extend2 > 0) return fail(VC_ERR_ARG, "gap extension penalties must be <= 0");
    for (const int32_t s : {p->match, p->mismatch, p->gap_open, p->gap_extend, p->gap_open2, p->gap_extend2})
        if (s < -128 || s > 127) return fail(VC_ERR_ARG, "scores must lie in -128..127 (spoa's int8_t parameters)");
    q.msa_flags = o ? o->flags : 0;
    if (q.msa_flags & ~(uint32_t)(VC_POA_MSA | VC_POA_MSA_CONSENSUS | VC_POA_COVERAGE)) return fail(VC_ERR_ARG, "unknown flag bits");
    if ((q.msa_flags & VC_POA_MSA_CONSENSUS) && !(q.msa_flags & VC_POA_MSA)) return fail(VC_ERR_ARG, "VC_POA_MSA_CONSENSUS needs VC_POA_MSA");
    if ((q.required & PoaRequest::GRAPH) && !q.graph) return fail(VC_ERR_ARG, "null graph output");
    if (((q.required & PoaRequest::STRAND) && !q.strand) || (q.strand && !q.strand->reversed)) return fail(VC_ERR_ARG, "null strand output (reversed is required)");
    if (q.required & PoaRequest::HAPS) {
        // vc_poa_run_haplotypes' own arguments, field by field in the struct's order, before the batch
        const vc_poa_hap_params* h = q.hap;
        if (h->max_haplotypes < 1 || h->max_haplotypes > VC_POA_HAP_MAX) return fail(VC_ERR_ARG, "max_haplotypes must lie in 1..VC_POA_HAP_MAX");
        if (h->min_reads < 1) return fail(VC_ERR_ARG, "min_reads must be >= 1");
        if (h->min_permille > 1000) return fail(VC_ERR_ARG, "min_permille must lie in 0..1000");
        if (h->rounds < 1) return fail(VC_ERR_ARG, "rounds must be >= 1");
        if (h->flags & ~(uint32_t)VC_POA_HAP_INDELS) return fail(VC_ERR_ARG, "unknown haplotype flag bits");
    }
    // the subtype and its scores (alignment_engine.cpp:59-69)
    int32_t g = p->gap_open, e = p->gap_extend, g2 = p->gap_open2, c = p->gap_extend2;
    const uint32_t gaps = g >= e ? 0 : (g <= g2 || e >= c ? 1 : 2);
    if (gaps == 0) e = g;
    else if (gaps == 1) { g2 = g; c = e; }
    q.route = q.graph ? graph_route() : 0;                                 // (vc_poa_run_align may ask for the tables too)
    LArgs a{};
    a.match = p->match; a.mismatch = p->mismatch; a.gap = g; a.gap_e = e; a.gap_q = g2; a.gap_c = c; a.gaps = gaps;
    a.msa = q.msa_flags; a.strand = q.strand ? 1 : 0; a.graph = q.route; a.state = q.state ? 1 : 0;
    a.profile = q.profile ? 1 : 0; a.haps = q.haps ? 1 : 0;
    if (o) { *o = vc_poa_msa_out{}; o->flags = q.msa_flags; }
    const bool owns = q.required || q.profile;
    if (owns) g_out.clear();                                               // what an earlier call handed out ends here
    const int rc = run_groups(p->device, p->algorithm, a, b, r, q);
    if (rc != VC_OK && owns) g_out.clear();
    if (rc != VC_OK) return rc;
    for (Stage* s : g_out.all()) s->publish(q, b);                         // every stage whose out-struct the call has, run or not
    return VC_OK;
}

// PoaRequest::required of the entries that add an input to another entry's call (vc_poa_run_from, _spans, _weighted): the entry
// the call would be without it -- the first of vc_poa_run_align, _graph, _strand, _msa, _gaps that it needs
uint32_t base_entry(const vc_batch* queries, const vc_poa_graph_out* g, const vc_poa_strand_out* s, const vc_poa_msa_out* o) {
    return queries ? PoaRequest::ALIGN : g ? PoaRequest::GRAPH : s ? PoaRequest::STRAND : o ? PoaRequest::MSA : 0u;
}

}  // namespace

extern "C" {

const char* vc_large_last_error(void) { return g_err.c_str(); }

void vc_large_release(void) { release_cache(); g_out.clear(); }

int vc_large_run(const vc_params* p, const vc_batch* b, vc_result* r) {
    if (!p || !b || !r || !r->cons_off || !r->status || (!r->cons && r->cons_cap)) return fail(VC_ERR_ARG, "null argument");
    if (const int rc = check_device(p->device, "the large-graph path", g_err)) return rc;
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
    return run_windows(p->device, a, b, caps, kn, r, PoaRequest{});
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
    return poa_run(&gp, b, r, PoaRequest{});
}

int vc_poa_run_gaps(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r) { return poa_run(p, b, r, PoaRequest{}); }

int vc_poa_run_msa(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o) { return poa_run(p, b, r, PoaRequest{PoaRequest::MSA, o}); }

int vc_poa_run_strand(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s) {
    return poa_run(p, b, r, PoaRequest{PoaRequest::STRAND, o, s});
}

int vc_poa_run_graph(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s,
                     vc_poa_graph_out* g) {
    return poa_run(p, b, r, PoaRequest{PoaRequest::GRAPH, o, s, g});
}

int vc_poa_run_align(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_strand_out* s, vc_poa_graph_out* g,
                     const vc_batch* q, vc_poa_align_out* a) {
    return poa_run(p, b, r, PoaRequest{PoaRequest::ALIGN, nullptr, s, g, q, a});
}

int vc_poa_run_from(const vc_poa_gap_params* p, const vc_poa_graph_in* from, const vc_batch* b, vc_result* r, vc_poa_msa_out* o,
                    vc_poa_strand_out* s, vc_poa_graph_out* g, vc_poa_state_out* st, const vc_batch* q, vc_poa_align_out* a) {
    if (st) *st = vc_poa_state_out{};                                      // a failed call leaves every pointer NULL
    if ((q == nullptr) != (a == nullptr)) return fail(VC_ERR_ARG, "the query batch and the align output go together");
    if (st && !g) return fail(VC_ERR_ARG, "the state output needs the graph output");
    PoaRequest rq{base_entry(q, g, s, o), o, s, g, q, a};
    rq.from = from; rq.state = st;
    return poa_run(p, b, r, rq);
}

int vc_poa_run_assign(const vc_poa_gap_params* p, const vc_poa_graph_in* from, const vc_batch* b, vc_result* r, const vc_batch* q,
                      vc_poa_assign_out* a) {
    if (a) { const uint32_t flags = a->flags; *a = vc_poa_assign_out{}; a->flags = flags; }   // a failed call leaves every pointer NULL
    if (!q || !a) return fail(VC_ERR_ARG, "the query batch and the assign output are both required");
    PoaRequest rq{PoaRequest::ASSIGN};
    rq.queries = q; rq.assign = a; rq.from = from;
    return poa_run(p, b, r, rq);
}

int vc_poa_run_spans(const vc_poa_gap_params* p, const vc_poa_span_in* spans, const vc_batch* b, vc_result* r, vc_poa_msa_out* o,
                     vc_poa_strand_out* s, vc_poa_graph_out* g) {
    PoaRequest rq{base_entry(nullptr, g, s, o), o, s, g};
    rq.spans = spans;
    return poa_run(p, b, r, rq);
}

int vc_poa_run_weighted(const vc_poa_gap_params* p, const vc_poa_weight_in* w, const vc_batch* b, vc_result* r, vc_poa_msa_out* o,
                        vc_poa_strand_out* s, vc_poa_graph_out* g, vc_poa_profile_out* prof) {
    PoaRequest rq{base_entry(nullptr, g, s, o), o, s, g};
    rq.weights = w; rq.profile = prof;
    return poa_run(p, b, r, rq);
}

void vc_poa_hap_default_params(vc_poa_hap_params* h) {
    if (h) *h = vc_poa_hap_params{2, 2, 250, 4, 0};
}

int vc_poa_run_haplotypes(const vc_poa_gap_params* p, const vc_poa_hap_params* h, const vc_batch* b, vc_result* r, vc_poa_hap_out* o) {
    PoaRequest q{PoaRequest::HAPS};
    q.hap = h; q.haps = o;
    return poa_run(p, b, r, q);
}

int vc_poa_run_correct(const vc_batch* b, const vc_poa_gap_params* p, const vc_poa_prune_params* pr, vc_result* r, vc_poa_correct_out* c) {
    PoaRequest q{PoaRequest::CORRECT};
    q.prune = pr; q.correct = c;
    return poa_run(p, b, r, q);
}

}  // extern "C"
