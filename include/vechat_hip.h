/* libvechat_hip.so -- C ABI of the MI355X-native replacement for VeChat's per-window hot path
 * (SPOA partial-order alignment + graph prune + consensus).
 *
 * Each entry point replaces a piece of the reference's C++ interface for this path; the
 * reference file:line it stands in for is cited next to it (paths relative to the reference
 * tree).  No C++ or torch types cross this boundary: plain pointers and sizes only.
 *
 * Threading and streams.  A vc_ctx is bound to one HIP device and must be driven by ONE host thread at a
 * time (the reference gives each worker its own spoa engine, src/polisher.cpp:186-190; its GPU shim gives
 * each batch processor its own stream, src/cuda/cudabatch.cpp:54).  Different contexts may be driven from
 * different threads at the same time.  What a context owns and what contexts share:
 *   - its own stream (vc_stream): H2D of vc_submit, D2H of vc_collect, fills;
 *   - the CHUNK STREAMS the kernels run on belong to the process: one set per device (up to 16, made on
 *     first use, never destroyed), used by every context of that device.  Two contexts that run at the
 *     same time interleave their chunks on those streams -- correct, results unchanged, but they share
 *     the device; nothing is gained over one context with batches queued behind each other;
 *   - host threads: one per chunk stream and context, started by the first vc_run, kept until vc_destroy
 *     (blocked on a condition variable while the context has nothing queued).
 * Pipelining inside one context.  A context holds TWO batches.  vc_run only queues the batch staged last
 * and returns; a vc_submit that follows copies the next batch in while that one runs; vc_collect hands out
 * the oldest run nobody has collected and waits for that run only.  So the loop of the reference's
 * accelerated polisher (fill the next batch while one computes, src/cuda/cudapolisher.cpp:246-277) is
 *     submit(b0) run   submit(b1) run   collect -> b0   submit(b2) run   collect -> b1   ...
 * on one thread, with H2D, kernels and D2H overlapping and no gap on the device between batches.  The
 * serial order (submit, run, [sync,] collect, submit ...) works as before and uses one batch slot.
 *
 * Environment variables.  This is every one the library reads; none is needed, and unset each leaves the default behaviour.
 * Read once per vc_create (vc_api.hip) -- a context keeps what it saw:
 *   VC_RESOLVE_FORCE_DFS   set: every end-cell tie is settled by the exact DFS as well (test_gpu::test_tie_resolution_by_exact_dfs)
 *   VC_HOST_THREADS=0      one host thread walks the chunk streams in lock-step, the scheduler of vc_debug_stop_after
 *                          (test_gpu::test_threaded_and_single_thread_host_schedulers_agree)
 *   VC_DT=0                global alignments on byte-packed rows stay on k_fwd instead of k_fwd_dt
 *                          (test_gpu::test_both_forward_kernels_give_the_same_bytes, tools/gpu_dt_ab.sh)
 *   VC_AUTO_ARENA=0        vc_submit does not make the workspace arena itself for the first large batch (development)
 *   VC_SCRATCH_CAP_GB=x    cap of the default workspace budget in GiB, x >= 1 (default 128; development, budget A/B runs)
 *   VC_TIME_SUBMIT         set: phases of vc_submit and of the arena's allocation on stderr (development)
 * Read by the host I/O (vc_io.cpp, vc_windows.cpp, vc_hostbuf.h) when a call needs them:
 *   VC_IO_THREADS=n        threads of the file readers and of the window builder (default: the host's cores, bounded)
 *   VC_IO_TIMING           set: phase times of the file readers on stderr (tools/gpu_files_host.sh)
 *   VC_HOSTBUF=0|1|2       host buffers: malloc / mmap + huge pages (default) / mmap; read once per process (tools/gpu_files_host.sh)
 * Read on every vc_large_run and vc_poa_run call (vc_large.hip, whose header describes them; tests/test_large_schedule.py):
 *   VC_LARGE_CAPS, VC_LARGE_ARENA_MB, VC_LARGE_MAT_MB, VC_LARGE_LOG (its lines: regrow, group, step, refuse, msa, graph, and for
 *   vc_poa_run_align with queries "vc_large: align jobs=J launches=K cells=C bytes=B", for vc_poa_run_assign "vc_large: assign ..."; done), VC_LARGE_GRAPH_WALK
 * Read on every vc_align call (vc_align.hip, whose header describes them; test knobs of tests/test_align.py):
 *   VC_ALIGN_BUDGET_MB=x   the chunk budget in MiB instead of half of the free device memory
 *   VC_ALIGN_MAX_MAT_MB=x  the envelope in MiB instead of a third of the device memory: an overlap whose stored matrix is larger
 *                          comes back with distance -1 and an empty CIGAR
 *   VC_ALIGN_LOG           set: one stderr line per chunk, "vc_align: chunk first=K pairs=N mat_dwords=D"
 */
#ifndef VECHAT_HIP_H_
#define VECHAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vc_ctx vc_ctx;

/* status codes returned by every call */
enum {
    VC_OK            = 0,
    VC_ERR_ARG       = -1,   /* bad argument / malformed batch                                  */
    VC_ERR_HIP       = -2,   /* a HIP runtime call failed (vc_last_error has the text)          */
    VC_ERR_NO_DEVICE = -3,   /* no gfx950 device visible: the product path has NO CPU fallback  */
    VC_ERR_STATE     = -4,   /* call out of order (e.g. vc_run before vc_submit)                */
    VC_ERR_CAPACITY  = -5    /* caller buffer too small                                         */
};

/* per-window status written by vc_run (vc_result.status) */
enum {
    VC_WIN_OK          = 0,  /* consensus produced; generate_consensus() would return true      */
    VC_WIN_UNPOLISHED  = 1,  /* < 3 sequences: backbone copied, returns false (window.cpp:188-192) */
    VC_WIN_OVERFLOW    = 2,  /* graph outgrew max_nodes/max_edges/stack: resubmit with larger caps, then vc_large_run */
    VC_WIN_UNSUPPORTED = 3,  /* reserved: no longer produced (every valid window is computed on the device) */
    VC_WIN_INVALID     = 4   /* input the reference would throw on (graph.cpp:191-231)          */
};

/* Replaces the constructor arguments the reference threads from main.cpp:46-61 through
 * createPolisher (src/polisher.cpp:59,140-157) into spoa::AlignmentEngine::Create
 * (polisher.cpp:186-190) and Window::generate_consensus (polisher.cpp:501-515). */
typedef struct vc_params {
    int32_t  device;                        /* HIP device ordinal                                  */
    int32_t  match, mismatch, gap;          /* -m -x -g (3,-5,-4)                                  */
    int32_t  sw_match, sw_mismatch, sw_gap; /* local engine hard-coded at window.cpp:326 (3,-5,-4) */
    double   min_confidence, min_support;   /* -d -s                                               */
    uint32_t num_prune;                     /* -k                                                  */
    int32_t  mode;                          /* 0 = haplotype overload (window.cpp:176)             */
    int32_t  trim;                          /* ignored in mode 0 (window.cpp:399)                  */
    int32_t  window_type;                   /* 0 kNGS / 1 kTGS (window.hpp:21-24)                  */
    uint32_t max_nodes;                     /* per-window graph capacity; 0 = derive from batch    */
    uint32_t max_edges;                     /* 0 = derive                                          */
    uint32_t chunk_windows;                 /* windows resident per pass; 0 = derive from memory   */
    uint64_t scratch_bytes;                 /* device scratch budget; 0 = 60 % of free memory, at most 128 GiB (VC_SCRATCH_CAP_GB) */
    int32_t  profile;                       /* 1 = bracket every kernel launch with HIP events, 2 = only the forward kernel's */
    uint32_t n_streams;                     /* chunks in flight on separate chunk streams (<= 16); 0 = chosen per batch: 8 from 12 288 windows up, else 4 */
} vc_params;

/* A batch of windows, the unit the reference's accelerated path fills with
 * CUDABatchProcessor::addWindow (src/cuda/cudabatch.hpp:39-59, cudabatch.cpp:79-135).
 * Sequence 0 of every window is the backbone (with its quality or the dummy '!' string,
 * polisher.cpp:397-400); sequences 1.. are the layers in the reference's `rank` order
 * (window.cpp:203-210) -- use vc_rank_layers() on the host to obtain it. */
typedef struct vc_batch {
    uint32_t        n_windows;
    const uint32_t* win_seq_off;   /* [n_windows+1]                                            */
    const uint64_t* seq_off;       /* [n_seqs+1] byte offsets into bases/quals                 */
    const uint32_t* seq_begin;     /* [n_seqs] positions_.first  (backbone: 0)                 */
    const uint32_t* seq_end;       /* [n_seqs] positions_.second (backbone: 0)                 */
    const uint8_t*  seq_has_qual;  /* [n_seqs] 0 = qualities_[i].first == nullptr              */
    const uint8_t*  bases;
    const uint8_t*  quals;         /* same offsets as bases; don't-care where has_qual == 0    */
    const uint8_t*  win_fasta;     /* [n_windows] window.cpp:223's `if_fasta` (vc_backbone_is_fasta) */
} vc_batch;

/* Result of a batch: Window::consensus() (window.hpp:43-45) of every window, concatenated, plus
 * the bool generate_consensus() returns (status VC_WIN_OK <=> true, VC_WIN_UNPOLISHED <=> false). */
typedef struct vc_result {
    uint64_t* cons_off;    /* [n_windows+1] out                         */
    uint8_t*  cons;        /* out, capacity cons_cap bytes              */
    uint64_t  cons_cap;
    uint8_t*  status;      /* [n_windows] out                           */
} vc_result;

typedef struct vc_stats {
    uint64_t cells;          /* sum over Align calls of graph_nodes * sequence_len  */
    uint64_t alignments;
    uint64_t dp_rows;
    uint64_t far_row_reads;  /* predecessor rows older than the LDS ring, read back from the H matrix */
    uint64_t trace_steps;    /* backtrack moves emitted                                               */
    uint64_t trace_spec;     /* ... of which confirmed in bulk by the first-in-edge speculation       */
    uint64_t trace_rounds;   /* speculation rounds (each: one batch of loads)                         */
    uint32_t n_classes;      /* kernel classes below                                            */
    double   ms[16];         /* accumulated HIP-event time per kernel class (profile=1)         */
    uint64_t launches[16];
    char     names[16][24];
    uint32_t max_nodes, max_edges, chunk_windows, n_streams;   /* what the context actually used */
    double   busy_ms[16];    /* per class: time during which at least one launch of it was running (the chunk streams overlap,  */
                             /* so a class's launches overlap each other and `ms` counts such time once per launch)             */
    uint64_t band_redo;      /* alignments whose backtrack left the stored band and were run again with whole rows              */
    uint64_t device_bytes;   /* device memory this context holds (workspaces + batch buffers)                                   */
    uint64_t fwd_shader_cycles, fwd_wall_ticks;   /* summed over the forward waves' row loops: shader cycles and 100 MHz ticks -- their ratio  */
                             /* x 100 is the shader clock in MHz the chip sustained under the job                                    */
} vc_stats;

/* -- lifecycle: stands in for createCUDABatch / ~CUDABatchProcessor (cudabatch.hpp:26,33) ------ */
int  vc_create(vc_ctx** out, const vc_params* p);
void vc_destroy(vc_ctx* ctx);
const char* vc_last_error(const vc_ctx* ctx);   /* ctx may be NULL: error of a failed vc_create */

/* -- batch: addWindow()... / generateConsensus() / reset() (cudabatch.hpp:39-59) --------------- */
int vc_submit(vc_ctx* ctx, const vc_batch* b);        /* validates, copies to HBM (H2D), retains nothing of b; does not wait for a batch
                                                         that is running unless the workspaces must grow for this one                 */
int vc_run(vc_ctx* ctx);                              /* queues the whole hot path for the batch staged last; returns at once          */
int vc_sync(vc_ctx* ctx);                             /* waits for every queued run                                                    */
/* The three calls below speak of the OLDEST run whose results have not been collected (none such: the latest run) and wait
 * for that run only; vc_collect / vc_collect_device mark it collected. */
int vc_result_windows(vc_ctx* ctx, uint32_t* n_windows);  /* windows of that batch                                 */
int vc_result_size(vc_ctx* ctx, uint64_t* cons_bytes);/* total consensus bytes                                 */
int vc_collect(vc_ctx* ctx, vc_result* r);            /* D2H of consensus + status                             */
/* device-side hand-over for the multi-GPU gather (RCCL lives in the caller, e.g. torch.distributed):
 * compacts the consensus bytes into caller-owned DEVICE memory. */
int vc_collect_device(vc_ctx* ctx, void* d_cons, uint64_t cons_cap, void* d_cons_off /*u64[n+1]*/,
                      void* d_status /*u8[n]*/);
int vc_get_stats(vc_ctx* ctx, vc_stats* s);
/* diagnostics: per-window (site << 16) | detail of the kernel that took the window out of VC_WIN_OK */
int vc_debug_errinfo(vc_ctx* ctx, uint32_t* out /*[n_windows]*/);
/* Test hooks for localising a divergence (tests/golden/stages.json): stop vc_run after a stage (kind 1 build layer `index`
 * added, 2 prune `index` done, 3 AddWeights round `index` done, 0 run to the end) and digest a window's graph / last alignment
 * where it stands, in the record format of the oracle's vco_window_stages.  Single-chunk batches. */
int vc_debug_stop_after(vc_ctx* ctx, uint32_t kind, uint32_t index);
int vc_debug_stage_digest(vc_ctx* ctx, uint32_t window, int with_pairs, uint64_t* out /*[8], [0..1] untouched*/);
/* development: the row records (16 B each) the next alignment of window w will use, after a stopped run (tools/gpu_rowstats.py) */
int vc_debug_rows(vc_ctx* ctx, uint32_t window, uint32_t* out, uint32_t cap_rows, uint32_t* nrows);
void* vc_stream(vc_ctx* ctx);                         /* the context's own hipStream_t (copies, fills); the kernels run on the process's chunk streams */
int   vc_set_profile(vc_ctx* ctx, int profile);       /* change vc_params.profile of a live context (0, 1, 2)  */
/* Always 0.  The library once carried measured-and-shelved experiments behind a build flag (the persistent build pipeline, an
 * LDS-row backtrack); they were removed, the export stays for callers that ask. */
int   vc_has_experiments(void);
/* Allocates the workspaces' memory now, in one piece (bytes = 0: the default budget, vc_params.scratch_bytes or 60 % of the free
 * memory up to 128 GiB), instead of under the first vc_submit; batches of any shape are then laid out inside it without further
 * allocations.  The counterpart of createCUDABatch sizing a batch's device memory at construction (mem_per_batch, src/cuda/cudapolisher.cpp:229-243):
 * a caller does it while its input is still being parsed.  Optional; without it vc_submit allocates what a batch needs. */
int   vc_reserve(vc_ctx* ctx, uint64_t bytes);
/* Changes the polishing parameters of a live context -- overload (mode), thresholds, prune rounds, trim, window type, scores: what differs
 * between the two rounds of the driver (scripts/vechat:59-93: round 1 `vechat_racon -f -p -d D -s S`, round 2 `-f [-u]`).  Device,
 * capacities, scratch budget and streams stay as created, workspaces stay where they are: one warm context serves both rounds and every
 * --split chunk, where a process per invocation (scripts/vechat:371-393) pays the start-up each time.  A batch staged before the call
 * must be submitted again. */
int   vc_set_polish_params(vc_ctx* ctx, const vc_params* params);
/* Gives the workspaces (and a reservation) back to the device; batch buffers and results stay.  The next vc_submit lays them out again.
 * For a caller that needs the memory for something else in between -- e.g. a second context for windows that overflowed. */
int   vc_release(vc_ctx* ctx);
/* The window type is known only after the reads are (Polisher::initialize, src/polisher.cpp:300-306); a context created before that
 * takes it here.  0 = kNGS, 1 = kTGS. */
int   vc_set_window_type(vc_ctx* ctx, int window_type);

/* -- host helpers that keep reference semantics on the host side of the boundary ---------------- */
/* rank[] as produced by window.cpp:203-210: rank[0]=0, rank[1..] = std::sort of 1..n-1 by begin
 * (same libstdc++ introsort => same permutation for ties). */
void vc_rank_layers(const uint32_t* begins, uint32_t n_seqs, uint32_t* rank_out);
/* window.cpp:223: `qualities_.front().first == std::string(len,'!')` -- a C-string comparison that
 * reads up to the NUL of the buffer `quality` points into. */
int  vc_backbone_is_fasta(const char* quality_cstr, uint32_t backbone_len);
/* graph.cpp:165-170 quality -> weight table as computed by this host's libm */
void vc_weight_lut(uint32_t lut[256]);

/* -- synthetic windows (SURVEY 8d generator; used by bench.py and the tests) -------------------- */
typedef struct vc_synth_cfg {
    uint64_t seed;
    uint32_t backbone_len;      /* L                                   */
    uint32_t n_layers;          /* D                                   */
    double   error_rate;        /* total per-base error                */
    double   frac_ins, frac_del, frac_sub;   /* split of the error      */
    double   frac_partial;      /* fraction of layers that are partial-span */
    int32_t  fastq;             /* 1 = layers carry qualities          */
    int32_t  backbone_fastq;    /* 1 = backbone has real quality, 0 = dummy '!' (FASTA target) */
    int32_t  n_haplotypes;      /* 1 or 2: reads drawn from this many variants of the truth    */
    double   snp_rate;          /* divergence between haplotypes       */
} vc_synth_cfg;

typedef struct vc_synth vc_synth;
/* generates windows [first, first+n) of the stream defined by cfg; layers are stored in rank order */
vc_synth* vc_synth_generate(const vc_synth_cfg* cfg, uint64_t first, uint32_t n, uint32_t n_threads);
void      vc_synth_batch(const vc_synth* s, vc_batch* out);   /* pointers stay owned by s */
uint64_t  vc_synth_n_seqs(const vc_synth* s);
/* [n_seqs] index each stored sequence had in add_layer() order (before the rank sort) */
const uint32_t* vc_synth_orig_index(const vc_synth* s);
uint64_t  vc_synth_n_bytes(const vc_synth* s);
void      vc_synth_free(vc_synth* s);

/* ------------------------------------------------------------------------------------------------
 * Window assembly and stitching (host only).  Stands in for the part of
 * Polisher::initialize that turns overlaps into windows (src/polisher.cpp:389-462, with the breaking
 * points of src/overlap.cpp:222-292 computed from a CIGAR string) and for the stitching loop of
 * Polisher::polish (src/polisher.cpp:520-547).  Sequences 0..n_targets-1 are the targets; overlaps are
 * taken in the order given (it decides the order of a window's layers before the rank sort).
 * ------------------------------------------------------------------------------------------------ */
typedef struct vc_wb vc_wb;
vc_wb*      vc_wb_create(uint32_t window_length, double quality_threshold);
void        vc_wb_destroy(vc_wb* b);
const char* vc_wb_last_error(const vc_wb* b);
/* returns the sequence id (>= 0) or -1; quality may be NULL (FASTA) */
int         vc_wb_add_sequence(vc_wb* b, const char* name, const char* data, uint32_t length, const char* quality);
/* the same without a copy: data / quality stay the caller's and must outlive the builder (vc_io_load passes its record buffers) */
int         vc_wb_add_sequence_view(vc_wb* b, const char* name, uint32_t name_len, const char* data, uint32_t length, const char* quality);
int         vc_wb_set_targets(vc_wb* b, uint32_t n_targets);
/* coordinates as in a PAF/SAM record: q_* on the read's forward strand, strand != 0 = reverse complement */
int         vc_wb_add_overlap(vc_wb* b, uint32_t q_id, uint32_t t_id, int strand, uint32_t q_begin, uint32_t q_end,
                              uint32_t q_length, uint32_t t_begin, uint32_t t_end, const char* cigar);
/* n overlaps at once, kept in the order given (their breaking points are computed on several threads) */
int         vc_wb_add_overlaps(vc_wb* b, uint64_t n, const uint32_t* q_id, const uint32_t* t_id, const uint8_t* strand, const uint32_t* q_begin,
                               const uint32_t* q_end, const uint32_t* q_length, const uint32_t* t_begin, const uint32_t* t_end,
                               const char* const* cigar);
uint32_t    vc_wb_n_breaking_points(const vc_wb* b, uint32_t overlap);
void        vc_wb_breaking_points(const vc_wb* b, uint32_t overlap, uint32_t* t_pos, uint32_t* q_pos);
/* fills `out` with arrays owned by the builder (valid until the next build / destroy): every window of every
 * target in order, layers in the reference's rank order */
int         vc_wb_build(vc_wb* b, vc_batch* out);
/* The same in two steps, for a caller that hands a large input to the device in slices (vc_submit of slice i + 1 while slice i runs): _begin
 * lays the whole batch out (every offset and buffer of `out` is final, the windows' bytes are not written yet), _fill writes the windows
 * [w_lo, w_hi).  A slice may be submitted once its windows are filled; filling the next one overlaps the device, as the reference's
 * accelerated polisher fills its next batch while one computes (src/cuda/cudapolisher.cpp:246-277). */
int         vc_wb_build_begin(vc_wb* b, vc_batch* out);
int         vc_wb_build_fill(vc_wb* b, uint32_t w_lo, uint32_t w_hi);
/* add_layer() index (0 = backbone) of every stored sequence of the last build, i.e. the rank permutation */
const uint32_t* vc_wb_seq_orig(const vc_wb* b);
uint32_t    vc_wb_n_windows(const vc_wb* b);
uint32_t    vc_wb_window_target(const vc_wb* b, uint32_t w);
uint32_t    vc_wb_window_rank(const vc_wb* b, uint32_t w);
void        vc_wb_window_ids(const vc_wb* b, uint32_t* target /*[n_windows]*/, uint32_t* rank /*[n_windows]*/);
/* per-target concatenation of the window results with the LN/RC/XC tags; fragment_correction adds the "r" */
int         vc_wb_stitch(vc_wb* b, const vc_result* res, int drop_unpolished, int fragment_correction);
uint32_t    vc_wb_n_polished(const vc_wb* b);
const char* vc_wb_polished_name(const vc_wb* b, uint32_t i);
const char* vc_wb_polished_data(const vc_wb* b, uint32_t i, uint64_t* length);

/* ------------------------------------------------------------------------------------------------
 * File formats (host only).  Stands in for what Polisher::initialize does with bioparser before a window
 * exists (src/polisher.cpp:77-138 parser selection, :207-352 loading and filtering) and for the record constructors of
 * src/sequence.cpp:19-42 and src/overlap.cpp:14-110.  vechat_amd/csrc/vc_io.cpp.
 * ------------------------------------------------------------------------------------------------ */
typedef struct vc_seqset vc_seqset;      /* the records of one FASTA / FASTQ (.gz) file */
typedef struct vc_ovlset vc_ovlset;      /* the records of one MHAP / PAF / SAM (.gz) file */
/* Always returns a set; vc_seqset_error() != NULL says what went wrong.  keep_names: NULL, or '\n'-separated names -- the other
 * records are passed over.  names_only: names and lengths, no data (a rank of a multi-GPU run plans with that). */
vc_seqset*      vc_io_read_sequences(const char* path, const char* keep_names, int names_only);
void            vc_seqset_free(vc_seqset* s);
const char*     vc_seqset_error(const vc_seqset* s);
uint64_t        vc_seqset_size(const vc_seqset* s);
const uint64_t* vc_seqset_name_off(const vc_seqset* s);   /* [n+1] into vc_seqset_names */
const char*     vc_seqset_names(const vc_seqset* s);
const uint64_t* vc_seqset_data_off(const vc_seqset* s);   /* [n+1] into vc_seqset_data / vc_seqset_qual */
const char*     vc_seqset_data(const vc_seqset* s);       /* upper-cased (sequence.cpp:19-42) */
const char*     vc_seqset_qual(const vc_seqset* s);       /* NULL when no record has a quality string */
const uint8_t*  vc_seqset_has_qual(const vc_seqset* s);   /* [n]; an all-'!' quality string counts as none */
const uint64_t* vc_seqset_lengths(const vc_seqset* s);    /* [n] */
typedef struct {
    const char* q_name; uint32_t q_name_len;              /* not NUL-terminated */
    const char* t_name; uint32_t t_name_len;
    uint8_t  by_index;                                    /* MHAP: q_index / t_index are positions in the reads / targets files */
    uint32_t q_index, t_index;
    uint8_t  strand;                                      /* 1 = reverse complement */
    uint32_t q_begin, q_end, q_length, t_begin, t_end, length;
    double   error;                                       /* 1 - min(spans) / max(spans) (overlap.cpp:21-26) */
    const char* cigar;                                    /* NULL: none yet (plain PAF, MHAP) */
    uint8_t  dropped;                                     /* could not be aligned (vc_ovlset_set_cigar(.., NULL)) */
} vc_overlap_rec;
vc_ovlset*  vc_io_read_overlaps(const char* path);        /* format from the extension, like the reference */
void        vc_ovlset_free(vc_ovlset* o);
const char* vc_ovlset_error(const vc_ovlset* o);
uint64_t    vc_ovlset_size(const vc_ovlset* o);
int         vc_ovlset_get(const vc_ovlset* o, uint64_t i, vc_overlap_rec* out);
int         vc_ovlset_set_cigar(vc_ovlset* o, uint64_t i, const char* cigar);
/* Planning for one rank of a multi-GPU run, on names, lengths and overlap records only (targets / reads may be names-only sets):
 * cost[k] = length of target k + the target bases its overlaps cover; and the '\n'-separated names (malloc'ed, vc_io_free) a rank
 * that owns targets [t_lo, t_hi) must load -- those targets and the queries of the overlaps on them. */
int         vc_io_target_cost(const vc_ovlset* o, const vc_seqset* targets, double* cost /*[targets]*/);
char*       vc_io_rank_names(const vc_ovlset* o, const vc_seqset* targets, const vc_seqset* reads, uint64_t t_lo, uint64_t t_hi, uint64_t* n_names);
void        vc_io_free(void* p);
/* Polisher::initialize, fragment-correction mode: every target, every read (a read that is also a target shares its record),
 * every overlap that survives the filters, into the window builder.  Returns the number of overlaps kept, -1 on error. */
int64_t     vc_io_load(vc_wb* builder, const vc_seqset* targets, const vc_seqset* reads, vc_ovlset* overlaps, double error_threshold,
                       int allow_empty, int* window_type, char* err, uint64_t err_cap);

/* ------------------------------------------------------------------------------------------------
 * Overlap alignment on the device.  Stands in for the edlib call the reference makes
 * for overlaps without a CIGAR (src/overlap.cpp:205-220): global unit-cost alignment with path, returned
 * as an edlib-standard CIGAR (M / I / D).  The path is optimal; which of several optimal paths is returned
 * is this library's choice (diagonal, then insertion, then deletion, from the end), not edlib's; the rule makes the
 * path unique, and tests/test_align.py pins it against a CPU DP.
 * q / t hold the pieces to align back to back (the query piece already oriented as it aligns);
 * Any length: scores are kept relative per 2048-column tile.  An overlap whose stored matrix would not fit the
 * device memory is not aligned: its distance comes back as -1 and its CIGAR empty; the others are unaffected.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t n;
    const uint64_t* q_off;   /* [n+1] */
    const uint8_t*  q;
    const uint64_t* t_off;   /* [n+1] */
    const uint8_t*  t;
} vc_align_batch;
int         vc_align(int device, const vc_align_batch* b, char* cigar, uint64_t cigar_cap, uint64_t* cigar_off,
                     int32_t* edit_distance);
const char* vc_align_last_error(void);
/* the aligner keeps its (large) matrix buffer between calls; this gives it back */
void        vc_align_release(void);

/* ------------------------------------------------------------------------------------------------
 * The large-graph path: windows the fast path hands back as VC_WIN_OVERFLOW (a graph beyond max_nodes / max_edges after
 * the capacity retries -- 16-bit ids, at most 59 968 nodes / 32 000 edges -- or a layer too long for k_addaln's LDS notes).
 * The same per-window algorithm with 32-bit ids and int32 scores on tables in HBM sized per window (grown and run again
 * when they fill): byte-identical results, no size limit but the device memory, and much slower per window than the fast
 * path.  A caller runs its overflowed windows through it where the reference's accelerated polisher runs them on the CPU
 * (src/cuda/cudapolisher.cpp:355-379).
 * Synchronous: computes every window of b and fills r like vc_collect (cons_cap >= the batch's bases is always enough);
 * statuses VC_WIN_OK / UNPOLISHED / INVALID as vc_collect, VC_WIN_OVERFLOW only for a window the device memory cannot hold
 * at all.  Honours device, the scores, mode, the thresholds, num_prune, trim and window_type; the capacity fields are ignored.
 * ------------------------------------------------------------------------------------------------ */
int         vc_large_run(const vc_params* p, const vc_batch* b, vc_result* r);
const char* vc_large_last_error(void);
/* the large path keeps its window tables and matrix buffer between calls; this gives them back (vc_poa_run's too: they share them) */
void        vc_large_release(void);

/* ------------------------------------------------------------------------------------------------
 * Consensus of read groups (POA groups).  Stands in for spoa's public flow, the general engine the reference vendors beneath its
 * windows (vendor/spoa; the flow of vendor/spoa/test/spoa_test.cpp:38-52 and of spoa's command line, src/main.cpp:270-323 with
 * -r 0), once per group of a batch:
 *     auto engine = spoa::AlignmentEngine::Create(algorithm, match, mismatch, gap);    alignment_engine.hpp:16-20, .cpp:15-70
 *     for every sequence, in the order given:
 *         graph.AddAlignment(engine->Align(sequence, graph), sequence[, quality]);      graph.cpp:132-300
 *     graph.GenerateConsensus();                                                         graph.cpp:450-459
 * A group is a window of vc_batch: win_seq_off delimits the groups, and a group may hold no sequence (empty consensus).  A
 * sequence with seq_has_qual takes the quality overload (weights as vc_weight_lut, the vendored graph.cpp:160-171), the others
 * weight 1; an empty sequence adds nothing (graph.cpp:187-190).  seq_begin, seq_end and win_fasta may be NULL and are ignored,
 * and so may quals when no sequence has a quality: no window rule applies (rank order, spans, subgraphs, "< 3 sequences",
 * prune, trim, window type).  Linear gaps (spoa's kLinear: e = q = c = g); vc_poa_run_gaps below takes affine and convex ones.
 * Synchronous, on the large-graph path's kernels (schedule 2 in vc_large.hip) and its buffer cache: fills r like vc_large_run
 * (cons_cap >= the batch's bases is always enough).  Status per group: VC_WIN_OK; VC_WIN_INVALID where the reference throws (the
 * group is left out, the others are computed); VC_WIN_OVERFLOW for a group the device memory cannot hold at all.
 * Envelope: sequences shorter than 65 535 bases; scores in -128..127 (spoa takes them as int8_t); otherwise the device memory.
 * Arguments are checked before the device is touched -- NULL pointers, algorithm outside 0..2, gap > 0 (alignment_engine.cpp:46-49),
 * a score outside -128..127, offsets that do not start at 0 or decrease, a sequence of 65 535 bases or more: VC_ERR_ARG -- and
 * only then the device: VC_ERR_NO_DEVICE without a gfx950 device.  vc_poa_last_error has the text of the last failure.
 * ------------------------------------------------------------------------------------------------ */
typedef struct vc_poa_params {
    int32_t device;
    int32_t algorithm;              /* 0 local (kSW), 1 global (kNW), 2 semi-global (kOV): spoa::AlignmentType   */
    int32_t match, mismatch, gap;   /* linear gaps (kLinear); gap <= 0 as spoa requires (alignment_engine.cpp:46-49) */
} vc_poa_params;
int         vc_poa_run(const vc_poa_params* p, const vc_batch* b, vc_result* r);
const char* vc_poa_last_error(void);

/* Affine and convex gaps: the same flow with the engine of
 *     spoa::AlignmentEngine::Create(algorithm, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)
 * whose subtype is chosen as alignment_engine.cpp:59-69 does: gap_open >= gap_extend selects linear gaps (with gap_extend =
 * gap_open), else gap_open <= gap_open2 or gap_extend >= gap_extend2 selects affine gaps (gap_open2 = gap_open, gap_extend2 =
 * gap_extend), else convex gaps (the better of two affine models).  spoa's own command line defaults are -g -8 -e -6 -q -10 -c -4:
 * convex.  Everything else as vc_poa_run: the batch, the result, the statuses, the envelope, vc_poa_last_error.  A parameter set
 * that selects linear gaps computes what vc_poa_run computes with gap = gap_open; only WorstCaseAlignmentScore, whose "possible
 * overflow" refusal (VC_WIN_INVALID) spoa takes from all four gap scores, may differ, on graphs of millions of nodes.
 * Affine alignments hold 3 int32 matrices (H, F, E), convex ones 5 (H, F, E, O, Q) of (nodes + 1) x (length + 1) cells each, on
 * the device.  Checked before the device, in spoa's order: NULL pointers, algorithm outside 0..2, gap_open or gap_open2 > 0,
 * gap_extend or gap_extend2 > 0, any of the six scores outside -128..127, then the batch as vc_poa_run: VC_ERR_ARG; then
 * VC_ERR_NO_DEVICE without a gfx950 device. */
typedef struct vc_poa_gap_params {
    int32_t device;
    int32_t algorithm;              /* 0 local (kSW), 1 global (kNW), 2 semi-global (kOV)                           */
    int32_t match, mismatch;
    int32_t gap_open, gap_extend;   /* spoa's g and e                                                               */
    int32_t gap_open2, gap_extend2; /* spoa's q and c (the second affine model of convex gaps)                      */
} vc_poa_gap_params;
int         vc_poa_run_gaps(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r);

/* The multiple sequence alignment and the per-base coverage of every group: beside the consensus, what
 *     graph.GenerateMultipleSequenceAlignment(include_consensus)                         graph.cpp:393-448 (spoa -r 1 / -r 2)
 *     graph.GenerateConsensus(&summary, false)                                           graph.cpp:461-485
 * return for the graph of the same flow.  p, b and r as vc_poa_run_gaps (a parameter set that selects linear gaps gives
 * vc_poa_run's bytes); o->flags selects the outputs and is the only field read:
 *     VC_POA_MSA            one row per sequence that was added, in the order given: '-' or the sequence's base per column
 *     VC_POA_MSA_CONSENSUS  (with VC_POA_MSA) one more row, the last, with the consensus
 *     VC_POA_COVERAGE       per consensus base, the number of sequences through its node and the nodes aligned to it
 * With flags == 0 the call is vc_poa_run_gaps: no labels kept, no extra kernel, every pointer of o NULL.
 * An empty sequence is never added (graph.cpp:187-190) and has no row, so row_member names the group member of every row
 * (index within the group; VC_POA_ROW_CONSENSUS for the consensus row).  A group that is VC_WIN_INVALID or VC_WIN_OVERFLOW has
 * n_rows = 0; a group without a non-empty sequence is VC_WIN_OK with row_size 0 and no row, or with VC_POA_MSA_CONSENSUS the one
 * consensus row of length 0, as the reference returns it.
 * Row i of group w is the row_size[w] bytes at rows + row_off[w] + i * row_size[w] (not NUL-terminated; blocks follow no
 * order and other bytes lie between them); its member is row_member[member_off[w] + i]; the coverage of consensus base k of
 * group w is coverage[r->cons_off[w] + k].
 * Lifetime: the library owns every array o points to.  They stay valid until the next vc_poa_* or vc_large_* call or
 * vc_large_release, whichever comes first (one set per process; like the buffer cache it is not thread-safe); copy what
 * must live longer.  A failed call leaves every pointer NULL.
 * Checked before the device, in this order: as vc_poa_run_gaps up to the scores, then flag bits other than the three above or
 * VC_POA_MSA_CONSENSUS without VC_POA_MSA, then the batch: VC_ERR_ARG. */
#define VC_POA_MSA            1u
#define VC_POA_MSA_CONSENSUS  2u
#define VC_POA_COVERAGE       4u
#define VC_POA_ROW_CONSENSUS  0xFFFFFFFFu
typedef struct vc_poa_msa_out {
    uint32_t flags;                 /* in: VC_POA_* bits                                                            */
    uint32_t n_groups;              /* out: b->n_windows                                                            */
    const uint32_t* n_rows;         /* [n_groups]                                                                   */
    const uint32_t* row_size;       /* [n_groups] columns of the group's alignment                                  */
    const uint64_t* row_off;        /* [n_groups] offset of the group's row block in rows                           */
    const uint64_t* member_off;     /* [n_groups + 1] first entry of the group in row_member (prefix sums of n_rows) */
    const uint32_t* row_member;     /* [member_off[n_groups]]                                                       */
    const uint8_t*  rows;
    uint64_t        rows_bytes;     /* bytes behind rows                                                            */
    const uint32_t* coverage;       /* [r->cons_off[n_groups]], or NULL without VC_POA_COVERAGE                     */
} vc_poa_msa_out;
int         vc_poa_run_msa(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o);

/* Strand-ambiguous groups: spoa's `-s` (src/main.cpp:287-304).  Every sequence, sequence 0 and empty ones included, is aligned
 * to the graph twice, as given and reverse-complemented, and the better strand is added:
 *     score = 0;     alignment     = Align(data, graph, &score);
 *     ReverseAndComplement();                                             biosoup/sequence.hpp:55-77
 *     score_rev = 0; alignment_rev = Align(data, graph, &score_rev);
 *     score >= score_rev ? ReverseAndComplement() again, keep `alignment` : keep `alignment_rev`
 * A score is the value of the end cell; it stays 0 where the engine does not write it: against the empty graph, for an empty
 * sequence, and where a local alignment finds no positive cell.
 * The tie rule: score == score_rev keeps the forward strand, so a sequence meeting the empty graph, an empty one and a
 * reverse-palindromic one are never reported reversed.
 * The complement is chosen on the upper-cased byte and is upper case: A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H; S, W, N
 * and every other byte stay as they are, in their own case.  The round-trip rule: a kept forward strand has been complemented
 * twice, which is not the identity -- u / U become T, lower-case a c g t r y k m b d h v become upper case (s, w, n keep their
 * case).  Its alignment was computed on the bytes as given; the nodes it adds, the consensus and the rows carry the
 * round-tripped bytes.  A kept reverse strand is added with its quality string reversed.  Rows show the kept bytes.
 * p, b, r and o as vc_poa_run_msa (o may be NULL: the consensus only); s is caller-owned, one entry per sequence of the batch
 * (b->win_seq_off[n_windows]), in batch order.  Groups that are not VC_WIN_OK have zeros in s.  Both strands' forward passes run
 * in one launch, each with a matrix of its own, so a step needs twice vc_poa_run_msa's matrix memory; the graph stages run once.
 * Checked before the device, in this order: as vc_poa_run_msa up to the flags, then s and s->reversed, then the batch:
 * VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these. */
typedef struct vc_poa_strand_out {
    uint8_t* reversed;              /* 1: the reverse complement was kept (required)                                */
    int32_t* score;                 /* spoa's *score of the forward strand (may be NULL)                            */
    int32_t* score_rev;             /* and of the reverse strand (may be NULL)                                      */
} vc_poa_strand_out;
int         vc_poa_run_strand(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s);

/* The partial order graph of every group: beside the consensus, what spoa's command line prints with -r 3 / -r 4 (PrintGfa,
 * src/main.cpp:120-200) and with -d (Graph::PrintDot, src/graph.cpp:746-803) -- nodes, weighted edges, aligned nodes, the path of
 * every sequence and the consensus path -- as tables, compacted on the device (k_lg_graph in vc_large.hip).
 * p, b and r as vc_poa_run_gaps.  o may be NULL; otherwise it is vc_poa_run_msa's and the alignment of the same graph comes with
 * it.  s NULL is the plain flow; otherwise it is vc_poa_run_strand's and the groups are built with spoa's -s.
 * The id rule: a node id is spoa's Node::id -- 0-based, in creation order (graph.cpp:73-76), local to its group.  GFA prints id + 1.
 * The layout, per batch, group w of n = n_groups:
 *   nodes    n_nodes[w] of them; node i of group w is entry node_off[w] + i of node_base (the decoded byte, graph.decoder(code)),
 *            of node_cons_pos (k: the node is consensus_[k]; -1: it is not on the consensus -- GFA's ic:Z:true, main.cpp:135-138,
 *            and dot's colours, graph.cpp:755-760,777) and of rank_to_node (the topological order, Graph::rank_to_node()).
 *   edges    out_off holds n_nodes[w] + 1 entries per group, node i's at out_off[node_off[w] + w + i]: its out-edges are
 *            edge_head[k] / edge_weight[k] (int64, Edge::weight) for k from that entry up to the next one.  Every edge of the graph
 *            appears once, ordered by tail id and then by position in the tail's out-list: the order in which PrintGfa and
 *            PrintDot print them (main.cpp:141-164, graph.cpp:764-783).  The group's edges are the k from out_off[node_off[w] + w]
 *            up to out_off[node_off[w + 1] + w].
 *   aligned  the pairs k in aligned_off[w] .. aligned_off[w + 1]: nodes aligned_a[k] < aligned_b[k] are aligned to each other; ordered
 *            by a and then by a's aligned-node list, dot's order (graph.cpp:784-800).
 *   paths    the paths k in path_first[w] .. path_first[w + 1], one per sequence that was added, in the order added (sequences_):
 *            path_member[k] is the index of the group member (as row_member: an empty member is never added, graph.cpp:187-190,
 *            and has no path); its nodes are path_node[path_off[k] .. path_off[k + 1]), one per base, from sequences_[k] along
 *            Node::Successor(k) (main.cpp:166-176).  path_reversed[k] is 1 where the strand flow kept the reverse complement: the
 *            nodes are in graph order and spell the kept bytes; PrintGfa prints such a path backwards with '-' (main.cpp:178-187).
 *   cons_node[r->cons_off[w] + k] is the node of consensus base k (Graph::consensus()).
 * A group that is not VC_WIN_OK has no node and no path; so has a group without a non-empty sequence.
 * Lifetime: as vc_poa_msa_out -- the library owns every array, they stay valid until the next vc_poa_* or vc_large_* call or
 * vc_large_release, and a failed call leaves every pointer NULL.
 * Calls that do not ask for the graph are unchanged: this entry alone launches k_lg_graph and keeps what it needs.
 * Checked before the device, in this order: as vc_poa_run_msa up to the flags (o == NULL counts as flags 0), then g, then
 * s->reversed when s is given, then the batch: VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these. */
typedef struct vc_poa_graph_out {
    uint32_t n_groups;              /* out: b->n_windows                                                            */
    const uint32_t* n_nodes;        /* [n_groups]                                                                   */
    const uint64_t* node_off;       /* [n_groups + 1] prefix sums of n_nodes                                        */
    const uint8_t*  node_base;      /* [node_off[n_groups]]                                                         */
    const int32_t*  node_cons_pos;  /* [node_off[n_groups]]                                                         */
    const uint32_t* rank_to_node;   /* [node_off[n_groups]]                                                         */
    const uint64_t* out_off;        /* [node_off[n_groups] + n_groups] into edge_head / edge_weight                 */
    const uint32_t* edge_head;
    const int64_t*  edge_weight;
    const uint64_t* aligned_off;    /* [n_groups + 1] into aligned_a / aligned_b                                    */
    const uint32_t* aligned_a;
    const uint32_t* aligned_b;
    const uint64_t* path_first;     /* [n_groups + 1] first path of the group                                       */
    const uint32_t* path_member;    /* [path_first[n_groups]]                                                       */
    const uint8_t*  path_reversed;  /* [path_first[n_groups]]                                                       */
    const uint64_t* path_off;       /* [path_first[n_groups] + 1] into path_node                                    */
    const uint32_t* path_node;
    const uint32_t* cons_node;      /* [r->cons_off[n_groups]]                                                      */
    uint64_t        bytes;          /* copied out of the device for this call                                       */
} vc_poa_graph_out;
int         vc_poa_run_graph(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_msa_out* o /* may be NULL */,
                             vc_poa_strand_out* s /* NULL: the plain flow; else spoa's -s */, vc_poa_graph_out* g);

/* Queries against finished groups: spoa's other public result, `engine->Align(sequence, graph, &score)` for a sequence that is
 * NOT added -- the score and the (node id, position) alignment of a query against the graph of its group, for assigning reads to
 * families by score, genotyping held-out reads, or asking which strand a read fits.
 * p, b, r, s and g as vc_poa_run_graph (g may be NULL here: no graph tables): the groups are built exactly as that call builds
 * them and the consensus comes back as always.  q holds the queries: q->n_windows == b->n_windows, and window w of q lists the
 * queries of group w (it may be empty); only n_windows, win_seq_off, seq_off and bases of q are read.  Every query is aligned
 * against the finished graph of its group with the call's engine -- the type, scores and subtype rule of the build -- and nothing
 * is added, so a group's consensus, graph and other queries do not depend on it.  a->flags selects:
 *     VC_POA_ALIGN_PAIRS    the alignments (pair_off, pair_node, pair_pos), not only the scores: without it no backtrack runs
 *     VC_POA_ALIGN_STRANDS  every query as given and reverse-complemented (the byte rule of vc_poa_run_strand), the better kept:
 *                           score >= score_rev keeps the query as given (main.cpp:297), so ties, palindromes and empty
 *                           alignments are never reported reversed.  A query is never added, so no byte makes a round trip.
 * Semantics, from the scalar engine (sisd_alignment_engine.cpp): an empty query, or a group with an empty graph, has an empty
 * alignment and score 0 (VC_WIN_OK); so has a local alignment without a positive cell; where WorstCaseAlignmentScore makes spoa
 * throw for the query's length, that query alone is VC_WIN_INVALID; a query whose matrix the device cannot hold is
 * VC_WIN_OVERFLOW; a query of a group that is not VC_WIN_OK carries the group's status, score 0 and no pairs.
 * Query k of the batch (queries in q's order) has pairs pair_off[k] .. pair_off[k + 1]: pair_node is the node id as in
 * vc_poa_graph_out or -1 (the base is inserted), pair_pos the position in the query -- in the kept strand's bytes when
 * reversed[k] -- or -1 (the node is skipped); spoa's Alignment, in sequence order.
 * The stage runs per batch of resident groups after their build (k_lg_rows, k_lg_qfwd, k_lg_qback, k_lg_qpack in vc_large.hip):
 * every (group, query) pair is independent, so the forward passes fill as few launches as the matrix budget allows.
 * Lifetime: as vc_poa_msa_out -- the library owns every array of a, they stay valid until the next vc_poa_* or vc_large_* call
 * or vc_large_release, and a failed call leaves every pointer NULL.  A call whose query batch holds no sequence runs no stage.
 * Checked before the device, in this order: as vc_poa_run_graph with g == NULL allowed, the batch included; then a, then flag
 * bits other than the two above; then q, its arrays and its window count against b; then the query lengths (below 65 535):
 * VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these. */
#define VC_POA_ALIGN_PAIRS    1u
#define VC_POA_ALIGN_STRANDS  2u
typedef struct vc_poa_align_out {
    uint32_t flags;                 /* in: VC_POA_ALIGN_* bits                                                      */
    uint64_t n_queries;             /* out: sequences of the query batch                                            */
    const uint8_t*  status;         /* [n_queries]                                                                  */
    const int32_t*  score;          /* [n_queries] spoa's *score: 0 where spoa does not write it                    */
    const int32_t*  score_rev;      /* [n_queries], NULL without VC_POA_ALIGN_STRANDS                               */
    const uint8_t*  reversed;       /* [n_queries], NULL without VC_POA_ALIGN_STRANDS                               */
    const uint64_t* pair_off;       /* [n_queries + 1], NULL without VC_POA_ALIGN_PAIRS                             */
    const int32_t*  pair_node;      /* spoa's Alignment: node id as in vc_poa_graph_out, or -1                      */
    const int32_t*  pair_pos;       /* position in the query (in the kept strand's bytes when reversed), or -1      */
    uint64_t        bytes;          /* copied out of the device for this stage                                      */
} vc_poa_align_out;
int         vc_poa_run_align(const vc_poa_gap_params* p, const vc_batch* b, vc_result* r, vc_poa_strand_out* s /* may be NULL */,
                             vc_poa_graph_out* g /* may be NULL */, const vc_batch* q, vc_poa_align_out* a);

/* Haplotype-aware correction of every member of a group: VeChat's variation-aware flow (src/window.cpp:176-428 on the vendored
 * spoa's PruneGraph, LargestSubgraph, AddWeights and GenerateCorrectedSequence, graph.cpp:811-1179) for POA groups, where one
 * graph serves all its members.  The reference has no group form; the flow is this composition of its public functions:
 *   1 build     the loop of vc_poa_run_gaps, unchanged; beside it total += the member's length (no quality) or, per base in order,
 *               1 - 10^((33 - q) / 10) (window.cpp:283,295), in double, in member order;
 *   2 consensus GenerateConsensus() of the unpruned graph: r holds vc_poa_run_gaps's bytes for the same input;
 *   3 average   avg = 2.0 * total / L, times 1000 when the first non-empty member has a quality string (window.cpp:301-309); L is
 *               that member's length.  A group without a non-empty member is VC_WIN_OK with the empty consensus and corrections;
 *   4 prune     PruneGraph(0, min_confidence, min_support, avg), then LargestSubgraph();
 *   5 rounds    num_prune - 1 times: every member, in order, is aligned against the pruned graph with the call's own engine
 *               (algorithm, scores, gap model) and AddWeights adds weight 1 per base, or vc_weight_lut's with a quality
 *               (window.cpp:351-373; an empty alignment or member adds nothing; an edge it creates is seen by the members after
 *               it); then PruneGraph and LargestSubgraph again;
 *   6 correct   every member is aligned against the final graph with a local engine (kSW) of the call's scores and gap model, and
 *               its correction is GenerateCorrectedSequence(alignment): the decoded base of every pair with a node, in order.
 *               A member that aligns nowhere, or is empty, has the empty correction; it is not an error.
 * Unlike the window overload (vc_large_run, mode 0) there is no backbone, no spans or subgraph, no rank sort, no "< 3 sequences"
 * rule, every round uses the call's engine for every member, and the final engine is local with the call's scores, not 3 / -5 / -4.
 * The arguments, in this entry's own order: the batch and p as vc_poa_run_gaps, the thresholds (the reference's defaults are
 * 0.22 / 0.19 / 3), r as vc_poa_run_gaps, and c.  This call takes none of the other outputs: the alignment rows, the graph tables,
 * the strand flow and the queries stay with their own calls, on the unpruned graph.
 * c is library-owned as vc_poa_msa_out is: valid until the next vc_poa_* or vc_large_* call or vc_large_release; a failed call
 * leaves every pointer NULL.  Sequence s of the batch has status[s], score[s] (the local score of step 6; 0 where spoa leaves it
 * unwritten) and the bytes corr[corr_off[s] .. corr_off[s + 1]).  status: VC_WIN_OK; VC_WIN_INVALID where WorstCaseAlignmentScore
 * makes spoa throw for that member in step 6; VC_WIN_OVERFLOW for a member whose matrix the device cannot hold; the members of a
 * group that is not VC_WIN_OK carry the group's status, score 0 and no bytes.
 * Steps 1-5 run on schedule 2's kernels, one alignment per group and step; step 6 runs all members of all resident groups side by
 * side (k_lg_rows, k_lg_qfwd, k_lg_qback, k_lg_correct in vc_large.hip).
 * Checked before the device, in this order: as vc_poa_run_gaps, the batch included (pr and c count among the NULL pointers); then
 * num_prune == 0 (the reference's num_prune - 1 would wrap); then a min_confidence or min_support that is NaN or negative:
 * VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these. */
typedef struct vc_poa_prune_params {
    double   min_confidence, min_support;
    uint32_t num_prune;
} vc_poa_prune_params;
typedef struct vc_poa_correct_out {
    uint64_t n_seqs;                /* out: sequences of the batch                                                  */
    const uint8_t*  status;         /* [n_seqs]                                                                     */
    const int32_t*  score;          /* [n_seqs] the local score of the final alignment                              */
    const uint64_t* corr_off;       /* [n_seqs + 1]                                                                 */
    const uint8_t*  corr;           /* the corrected members, back to back                                          */
    uint64_t        bytes;          /* copied out of the device for this stage                                      */
} vc_poa_correct_out;
int         vc_poa_run_correct(const vc_batch* b, const vc_poa_gap_params* p, const vc_poa_prune_params* pr, vc_result* r,
                               vc_poa_correct_out* c);

/* Groups that go on from a stored graph: spoa's incremental flow -- AddAlignment on a live Graph, and Graph::save / load
 * (graph.hpp:196-300) -- for POA groups.  A call hands a group's graph out as tables (g and st), and a later call takes them back
 * (from), adds the new members of b to it and / or aligns queries against it, instead of building the group from nothing.
 * The state of a group is its vc_poa_graph_out tables plus one more, vc_poa_state_out: every node's full aligned list in list
 * order.  Everything later steps read follows from them: node ids and bases; each node's out-list (the edge order of out_off),
 * aligned list (al_off / al_node) and in-list -- a sequence meets a node once, so it creates at most one edge into a head, an
 * edge's first label is the sequence that created it, and replaying the paths in order rebuilds the in-lists and the labels --;
 * the edge weights; sequences_ (a path's first node and member); and spoa's coder / decoder, first appearance over the bytes the
 * paths spell in order.  aligned_a / aligned_b alone do not do: they keep only the larger ids of a node's list, and of a class
 * c0 < c1 < c2 the list of c2 is [c1, c0] or [c0, c1] depending on which node it was made against (graph.cpp:263-280); that order
 * drives later topological sorts and with them the rows and tie rules of later alignments.
 * from == NULL builds every group from nothing, as vc_poa_run_align (q, a given) or vc_poa_run_graph, _strand, _msa, _gaps (the
 * first that the given outputs need) does, to the launch and the log line when st is NULL too; a state is first obtained that way
 * with g and st.  Otherwise from->n_groups == b->n_windows and group w starts as graph w of `from` -- which may have no node -- and
 * window w of b lists its new members, possibly none; they are aligned and added in the order given with this call's engine.
 * r as vc_poa_run_gaps; a consensus may run through stored nodes, so cons_cap >= the batch's bases plus the stored graphs' nodes
 * is always enough.
 * The id rule: node ids are vc_poa_graph_out's, and the stored nodes keep theirs.  The members of b are numbered from
 * from->n_members[w] in row_member / path_member; earlier members keep their numbers, rows and paths (and path_reversed); the
 * caller's n_members for the next call is from->n_members[w] plus the members of window w of b, empty ones included.  s has one
 * entry per sequence of b only.  o, s, g, q and a behave as in vc_poa_run_msa / _strand / _graph / _align; any of o, s, g, st may
 * be NULL; q and a are both NULL or both given; st requires g.
 * The contract: for members m0 .. m(n-1) and any k, the tables and state after m0 .. m(k-1), passed back unmodified with
 * m(k) .. m(n-1) and the same parameters, give the consensus, rows, coverage, graph tables, state, strand choices and query
 * alignments of one call on m0 .. m(n-1), byte for byte.  The engine may differ between the calls, as in spoa; equality with the
 * one call is promised for identical parameters only.
 * vc_poa_run_correct has no `from` form: its average weight needs `total` over every member's bases and qualities
 * (window.cpp:283-309), and the graph does not hold them.
 * from is caller-owned and read during the call only: the arrays of a vc_poa_graph_out and a vc_poa_state_out in the same
 * layout (copy them first: this call's own outputs end the lifetime of the earlier call's).  st is library-owned, lifetime as
 * vc_poa_graph_out; a failed call leaves every pointer NULL.  g->bytes counts the graph tables alone and st->bytes the state
 * table, though one copy brings both out.
 * The checks keep every index on the device in range and every list well formed; they do not prove that the tables are a graph
 * this library could have written (weights, ranks and list orders are taken as given), and for tables it could not have
 * written the results are whatever the flow computes from them.
 * from is untrusted, and everything is checked on the host before the device is touched, in this order: q and a together, st
 * with g; then as vc_poa_run_align (or the entry the call stands for), the batch and the queries included; then from: the group
 * count against b; NULL offset tables, n_members or n_nodes; offsets that do not start at 0, decrease, or (path_off) do not
 * increase -- a path has a node --, node_off against n_nodes, a group of 2^31 nodes, edges, aligned cells or path entries, and
 * NULL tables where the offsets count an entry; every edge_head, al_node, path_node and rank_to_node below the group's n_nodes;
 * rank_to_node a permutation in which every edge runs forward; aligned lists without their own node or a node twice, and
 * symmetric, and never joined by an edge; every consecutive pair of a path an edge of the tail's out-list (the first with that
 * head), and every edge on some path -- which also refuses a second edge u -> v --; path_member below n_members (and n_members plus the
 * new members below 2^32 - 1): VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these. */
typedef struct vc_poa_state_out {          /* library-owned, lifetime as vc_poa_graph_out                                */
    const uint64_t* al_off;                /* [node_off[n_groups] + n_groups] per group n_nodes + 1 entries, laid out as out_off, into al_node */
    const uint32_t* al_node;               /* every node's aligned list, in list order                                   */
    uint64_t        bytes;                 /* copied out of the device for this table                                    */
} vc_poa_state_out;
typedef struct vc_poa_graph_in {           /* caller-owned: the arrays of a vc_poa_graph_out and a vc_poa_state_out, same layout */
    uint32_t n_groups;
    const uint32_t* n_members;             /* [n_groups] members the group has had so far, empty ones included           */
    const uint32_t* n_nodes;  const uint64_t* node_off;  const uint8_t* node_base;  const uint32_t* rank_to_node;
    const uint64_t* out_off;  const uint32_t* edge_head;  const int64_t* edge_weight;
    const uint64_t* al_off;   const uint32_t* al_node;
    const uint64_t* path_first; const uint32_t* path_member; const uint8_t* path_reversed;
    const uint64_t* path_off;   const uint32_t* path_node;
} vc_poa_graph_in;
int         vc_poa_run_from(const vc_poa_gap_params* p, const vc_poa_graph_in* from /* NULL: from nothing */, const vc_batch* b,
                            vc_result* r, vc_poa_msa_out* o, vc_poa_strand_out* s, vc_poa_graph_out* g, vc_poa_state_out* st,
                            const vc_batch* q, vc_poa_align_out* a);

/* Queries assigned to groups: `engine->Align(sequence, graph, &score)` for every query against EVERY group, and per query the
 * best and the second group by score -- the family a read belongs to, and how far ahead of the runner-up it is.  With
 * vc_poa_run_align a caller has to copy every query into every group and reduce on the host, and every copy stores a full
 * matrix that nothing reads; here a pair costs a ring of the graph's live rows and the reduction runs on the device.
 * The groups are built as vc_poa_run_from builds them with the same p, from and b (from == NULL: from nothing, as
 * vc_poa_run_gaps), and r comes back as that call returns it.  Every sequence of q is a query against every group: of q only
 * the sequence count (win_seq_off[n_windows]; 0 when n_windows is 0), seq_off and bases are read, and its window boundaries
 * mean nothing.  a->flags selects:
 *     VC_POA_ASSIGN_STRANDS  every query as given and reverse-complemented, the rule of VC_POA_ALIGN_STRANDS (main.cpp:287-304:
 *                            score >= score_rev keeps the query as given), and the kept strand's score is the pair's score
 *     VC_POA_ASSIGN_SCORES   also the dense table: one score and one status per (query, group), query-major
 * The score, the strand choice and the status of pair (k, w) are exactly what vc_poa_run_align without VC_POA_ALIGN_PAIRS
 * reports for query k placed in group w: the empty query and the local alignment without a positive cell score 0; where
 * WorstCaseAlignmentScore makes spoa throw the pair is VC_WIN_INVALID; a pair whose rows the device cannot hold is
 * VC_WIN_OVERFLOW; the pairs of a group that is not VC_WIN_OK carry its status and score 0.
 * A pair is ranked when its group is VC_WIN_OK and has at least one node and the pair itself is VC_WIN_OK.  (A group with an
 * empty graph scores 0 for everything and would win every global assignment: it is scored, never ranked.)  best is the
 * highest ranked score, ties to the lower group index; second is the best over the other groups by the same rule.  status[k]
 * is VC_WIN_OVERFLOW if any pair of k overflowed, else VC_WIN_INVALID if any was invalid, else VC_WIN_OK; the ranked pairs are
 * reported either way.
 * The stage runs per batch of resident groups after their build (k_lg_rows, k_lg_slots, k_lg_sfwd, k_lg_assign in
 * vc_large.hip): row r of a graph is read by its successors only, so a forward pass that needs no backtrack keeps a row only
 * until the last of them is complete -- n_slots rows, the width of the graph's bubbles, instead of all of them -- and computes
 * the same cells with the same recurrence.
 * Lifetime and failure as vc_poa_align_out: the library owns every array of a until the next vc_poa_* or vc_large_* call or
 * vc_large_release, and a failed call leaves every pointer NULL.  A call with no query or no group runs no stage and returns
 * the arrays empty or filled with the "none" values below.
 * Checked before the device, in this order: q and a (both required); then as vc_poa_run_from with q and a given -- the batch,
 * the query batch's arrays and lengths, from --; then flag bits other than the two above: VC_ERR_ARG.  VC_ERR_NO_DEVICE only
 * after these. */
#define VC_POA_ASSIGN_STRANDS 1u
#define VC_POA_ASSIGN_SCORES  2u
typedef struct vc_poa_assign_out {
    uint32_t flags;                 /* in: VC_POA_ASSIGN_* bits                                                     */
    uint64_t n_queries;             /* out: sequences of the query batch                                            */
    uint32_t n_groups;              /* out: groups of the batch                                                     */
    const uint8_t*  status;         /* [n_queries]                                                                  */
    const int32_t*  best_group;     /* [n_queries] -1 where no pair was ranked                                      */
    const int32_t*  best_score;     /* [n_queries] 0 where no pair was ranked                                       */
    const int32_t*  second_group;   /* [n_queries] the best over the other groups, same rule, -1 where none         */
    const int32_t*  second_score;   /* [n_queries] 0 where none                                                     */
    const uint8_t*  reversed;       /* [n_queries] the strand kept against best_group, NULL without VC_POA_ASSIGN_STRANDS */
    const int32_t*  scores;         /* [n_queries * n_groups] query-major, NULL without VC_POA_ASSIGN_SCORES        */
    const uint8_t*  pair_status;    /* [n_queries * n_groups], NULL without VC_POA_ASSIGN_SCORES                    */
    uint64_t        bytes;          /* copied out of the device for this stage                                      */
} vc_poa_assign_out;
int         vc_poa_run_assign(const vc_poa_gap_params* p, const vc_poa_graph_in* from /* may be NULL */, const vc_batch* b,
                              vc_result* r, const vc_batch* q, vc_poa_assign_out* a);

/* Span-limited alignment of group members: spoa's Graph::Subgraph / UpdateAlignment (graph.cpp:640-745) for POA groups, as the
 * reference's Window::generate_consensus uses them (window.cpp:207-213) -- for groups whose members are shorter than their
 * locus: tiled amplicons, the reads that map to a contig, a long construct sequenced in pieces.  Against the whole graph such a
 * member costs rows it does not need, a global alignment of it is wrong, a local one loses its ends, and a repeat inside the locus
 * may attract it to the wrong copy.
 * p, b, r, o, s and g as vc_poa_run_graph (o, s and g may each be NULL).  spans holds one (begin, end) per sequence of b,
 * caller-owned and read during the call only.  The flow is spoa's own, per group and in the order given:
 *   1. sequence 0 is aligned against the (empty) graph and added; its own span entries are ignored;
 *   2. a later member whose begin == end == VC_POA_SPAN_NONE is aligned against the whole graph, as in every other entry;
 *   3. any other member is aligned against graph.Subgraph(begin, end, &map) with the call's engine and gap model -- the nodes from
 *      which `end` can be reached backwards over in-edges and aligned nodes without passing below id `begin` --, the alignment is
 *      mapped back with UpdateAlignment and added to the full graph with AddAlignment.  What of the member lies before or behind
 *      what the subgraph aligned becomes new chains, as AddAlignment makes them.
 * Coordinates: begin and end are inclusive positions on sequence 0 of the group.  A group is built from nothing here, so base k
 * of sequence 0 is node k (the id rule of vc_poa_run_graph) and the span is a pair of node ids.
 * The library applies no span rule of its own: racon's "within 1 % of both window ends counts as spanning" (window.cpp:207-208)
 * is the caller's to apply or not -- it says NONE or gives a span --, and the members stay in the order given, with no rank sort.
 * With s (spoa's -s) both strands of a member are aligned against the same subgraph and the better one is mapped back and added,
 * ties going forward; the span is in sequence 0's coordinates whichever strand is kept.
 * o and g describe the full graph, exactly as in vc_poa_run_msa / vc_poa_run_graph: a subgraph never shows.
 * An empty member adds nothing, with or without a span.
 * spans == NULL, or every entry VC_POA_SPAN_NONE, is the entry the same outputs would have selected -- the first of
 * vc_poa_run_graph (g), _strand (s), _msa (o), _gaps that they need --, byte for byte, launch for launch and log line for log
 * line: nothing of the spans reaches the device then.
 * Spans are untrusted: a bad node id on the device would be a fault.  Checked on the host before the device is touched, in this
 * order: as vc_poa_run_graph (with g == NULL counting as "no graph output", s and o likewise), the batch included; then the span
 * arrays (NULL beside a sequence); then, member by member in batch order, for every member but the first of its group whose span
 * is not NONE / NONE: never exactly one of the two entries NONE; begin <= end; end < the length of sequence 0 of its group.  A
 * violation is VC_ERR_ARG and vc_poa_last_error names the group and the member.  A group whose sequence 0 is empty therefore admits
 * no span.  VC_ERR_NO_DEVICE only after these.
 * Out of scope: spans for vc_poa_run_from (in a loaded graph a position on sequence 0 is not a node id without its path), for
 * vc_poa_run_correct (its rounds rebuild and renumber the graph) and for the queries of vc_poa_run_align. */
#define VC_POA_SPAN_NONE 0xFFFFFFFFu
typedef struct vc_poa_span_in { const uint32_t* begin; const uint32_t* end; } vc_poa_span_in;   /* [n_seqs of b], caller-owned */
int         vc_poa_run_spans(const vc_poa_gap_params* p, const vc_poa_span_in* spans /* NULL: no span */, const vc_batch* b, vc_result* r,
                             vc_poa_msa_out* o, vc_poa_strand_out* s, vc_poa_graph_out* g);   /* o, s, g may be NULL, as in vc_poa_run_graph */

/* Explicit weights and the per-base profile of the consensus: the two other AddAlignment overloads of spoa::Graph
 * (graph.hpp:142-170, graph.cpp:132-196) and GenerateConsensus(&summary, true) (graph.cpp:486-529).
 * p, b, r, o, s and g as vc_poa_run_graph (o, s, g and prof may each be NULL).
 * Weights.  w holds one mode per sequence of b, caller-owned and read during the call only:
 *   0  what vc_batch says: the quality overload where the member has a quality (vc_weight_lut), weight 1 for every base otherwise;
 *   1  seq_weight[s] for every base of the member (the uint32_t weight overload): "this read stands for 37 duplicates";
 *   2  base_weight[seq_off[s] + i] for base i (the std::vector weights overload).
 * They are exactly the reference's: the edge between bases i - 1 and i of a member gets weights[i - 1] + weights[i], computed in
 * uint32_t -- so it wraps modulo 2^32 -- and then added to the edge's int64_t weight (graph.cpp:125, 182-300).  Weight 0 is
 * legal.  An empty member adds nothing, whatever its mode.  With s (spoa's -s) a kept reverse strand is added with its weight
 * vector reversed, as its quality string is; a mode-1 member is unaffected.  spoa's "sequence and weights are of unequal size"
 * cannot be expressed in this layout.  Weights move edge weights, and with them the consensus; they enter no alignment score.
 * Profile.  prof, library-owned with the lifetime of vc_poa_msa_out, receives for every group the codes of its graph -- the
 * bytes in order of first appearance, spoa's decoder_ -- and a block of (n_codes + 1) rows of cons_len uint32_t: row k counts,
 * per consensus position, the members that carry code k in that position's column, the last row those that span it with a
 * gap (between two of their bases that lie on consensus columns; nothing before a member's first such base or behind its last).
 * Weights do not enter the counts.  The code rows sum to VC_POA_COVERAGE's figure but for one-base members, which Coverage() misses.  A group that is not
 * VC_WIN_OK has n_codes = 0 and an empty block; so has a VC_WIN_OK group without a non-empty member.  prof may be asked with or
 * without weights and with or without o, s and g.  A failed call leaves every pointer NULL.
 * w == NULL, or every mode 0, together with prof == NULL is the entry the same outputs would have selected -- the first of
 * vc_poa_run_graph (g), _strand (s), _msa (o), _gaps that they need --, byte for byte, launch for launch and log line for log
 * line: nothing of the weights reaches the device then.  base_weight is uploaded only when a member has mode 2.
 * Checked on the host before the device is touched, in this order: as vc_poa_run_graph (with g, s, o == NULL counting as "not
 * asked"), the batch included; then w->mode NULL (with w given, whatever the batch holds); then a mode above 2 on any member; then
 * seq_weight NULL beside a mode-1 member; then base_weight NULL beside a mode-2 member -- one kind after the other, and within a
 * kind the first member in batch order.  A violation is VC_ERR_ARG and vc_poa_last_error names the group and the member.
 * VC_ERR_NO_DEVICE only after these.
 * Out of scope: weights or the profile for vc_poa_run_from (stored paths carry no weights and their profile belongs to the call that built them).
 * Out of scope: weights or the profile for vc_poa_run_align (queries are not added, so they weigh nothing).
 * Out of scope: weights or the profile for vc_poa_run_correct (its rounds take the quality overload of add-weights only).
 * Out of scope: weights or the profile for vc_poa_run_spans (one extension per entry; the two do not combine yet). */
typedef struct vc_poa_weight_in {
    const uint8_t*  mode;         /* [n_seqs of b]  0: as vc_batch says (quality overload, or 1)
                                                    1: seq_weight[s] for every base (spoa's uint32_t weight overload)
                                                    2: base_weight[seq_off[s] + i]  (spoa's vector overload)          */
    const uint32_t* seq_weight;   /* [n_seqs], read where mode == 1; may be NULL if no member has mode 1                 */
    const uint32_t* base_weight;  /* at b->seq_off's offsets, read where mode == 2; may be NULL if no member has mode 2  */
} vc_poa_weight_in;               /* caller-owned, read during the call only */

typedef struct vc_poa_profile_out {   /* library-owned, lifetime as vc_poa_msa_out */
    uint32_t        n_groups;
    const uint32_t* n_codes;      /* [n_groups]  the graph's num_codes_                                                  */
    const uint64_t* code_off;     /* [n_groups + 1] into codes                                                           */
    const uint8_t*  codes;        /* decoder_[k] for k < n_codes[w]: the byte of row k, in order of first appearance     */
    const uint64_t* prof_off;     /* [n_groups] offset of the group's block in counts                                    */
    const uint32_t* counts;       /* block of (n_codes[w] + 1) rows x cons_len[w]; row k at prof_off[w] + k * cons_len;
                                     the last row counts gaps: summary[code * consensus_.size() + c], graph.cpp:488-517  */
} vc_poa_profile_out;

int         vc_poa_run_weighted(const vc_poa_gap_params* p, const vc_poa_weight_in* w /* NULL: none */, const vc_batch* b, vc_result* r,
                                vc_poa_msa_out* o, vc_poa_strand_out* s, vc_poa_graph_out* g, vc_poa_profile_out* prof /* o, s, g, prof may be NULL */);

/* ------------------------------------------------------------------------------------------------
 * Haplotypes of a POA group: how many alleles a group holds, their sequences, and which member belongs to which.
 * vc_poa_run_haplotypes builds every group exactly as vc_poa_run_gaps does -- r carries that call's consensus bytes and
 * statuses, unchanged -- and then splits the members of every VC_WIN_OK group by the library's own rule.  The rule is all
 * integer and every tie is decided; tests/poa_haplo_ref.py restates it and the device is pinned to that restatement.
 *
 * Terms.  S: the sequences that were added (empty members are not), labelled 0 .. S-1 in the order added.  C: the alignment
 * columns of vc_poa_run_msa.  node(s,c): the node of sequence s in column c, if it has one.  first(s), last(s): the lowest and
 * highest column of s.  sym(s,c): the code of node(s,c) where it exists; GAP where it does not and first(s) < c < last(s);
 * NONE otherwise.  Codes are the graph's, in order of first appearance of their byte.
 *   1 Counts.  n(c,a): the s with sym(s,c) = a, for every code a and for GAP.  span(c): the s with first(s) <= c <= last(s).
 *   2 Sites.   The alleles are the codes in code order; with VC_POA_HAP_INDELS GAP is an allele too and comes last.  Allele a
 *              qualifies at c when n(c,a) >= min_reads and 1000 * n(c,a) >= min_permille * span(c).  A column with at least two
 *              qualifying alleles is a site; its major allele is the qualifying one with the largest count, a tie going to the
 *              earlier allele, its minor allele the next by the same order.  Sites run in column order: m = 0 .. M-1.
 *   3 Votes.   v(s,m) = +1 where sym(s, column of m) is the major allele, -1 where it is the minor allele, 0 otherwise (another
 *              base, a GAP without the flag, a member that does not span the site).  agree(x,y) = sum over m of x[m] * y[m].
 *   4 Seeds.   seed_0 is the member with the most non-zero votes, a tie going to the smallest label; without a non-zero vote
 *              K = 1.  For k = 1 .. max_haplotypes - 1: d(s) = max over j < k of agree(v(s), v(seed_j)); the s with the smallest
 *              d(s), a tie going to the smallest label, is seed_k unless its d(s) >= 0, which ends the seeding.
 *   5 Rounds.  P_k = v(seed_k).  `rounds` times: every member joins the k with the largest agree(v(s), P_k), a tie going to the
 *              smallest k; then P_k[m] = sign of the sum of its members' votes at m (0 on a tie and for an empty cluster).  A
 *              round that moves no member ends the loop (the fixed point is the same).
 *   6 Small clusters.  The clusters with fewer than min_reads members are removed together, and their members join the
 *              surviving P_k they agree with best, a tie going to the smallest k; profiles are not recomputed.  If no cluster
 *              survives all members form one cluster.
 *   7 Order.   Haplotype ids run by size, largest first, a tie going to the cluster with the smaller smallest label.  A member
 *              that was never added (an empty one) has VC_POA_HAP_NONE.
 *   8 Consensus of haplotype k: spoa's GenerateConsensus (heaviest bundle with branch completion, graph.cpp) on the group's graph
 *              restricted to the members of k.  A node belongs when a member of k has it on its path, an edge when a member of k
 *              carries it; the weight of an edge is the sum over those members of w_s[i-1] + w_s[i] for the step i of the member's
 *              path that takes the edge (w: the build's own base weight, vc_weight_lut of the quality or 1: what AddEdge added
 *              for them).  The order of the nodes is the full graph's rank_to_node, every in-list keeps its order, and the
 *              out-degree is taken inside the restricted graph.  With K = 1 nothing is removed, so haplotype 0 is r's consensus.
 *
 * Out, per group w: n_haps[w] haplotypes at hap_first[w] ..; per haplotype h its member count hap_size[h] and its bytes
 * cons[cons_off[h] .. cons_off[h + 1]); per sequence of the batch hap_of; the sites of w at site_off[w] .. site_off[w + 1].
 * A group that is not VC_WIN_OK has no haplotype and no site and its members carry VC_POA_HAP_NONE; a group without a non-empty
 * member is VC_WIN_OK with one haplotype of zero members and the empty consensus.  The entry takes no spans, weights, strands,
 * queries or stored graphs.
 * One exception to "r unchanged": the stage needs, per group, a block and a scratch in device memory (4 bytes per member and
 * column for the node ids, one for the votes, and per haplotype a copy of the edge weights and the bundle's tables).  A single
 * group the device has no room for is VC_WIN_OVERFLOW in r with the empty consensus, as the other output stages
 * (vc_poa_run_msa, vc_poa_run_graph) report a group whose output they cannot hold, although vc_poa_run_gaps alone would
 * have computed it.
 * Argument checks before the device, in this order: those of vc_poa_run_gaps on p and r (o NULL and h NULL count as null
 * arguments); then the fields of h: max_haplotypes, min_reads, min_permille, rounds, unknown flag bits; then the batch:
 * VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these.
 * Not this stage: phasing across groups, sites with more than two alleles (the third allele votes 0), realignment per haplotype. */
#define VC_POA_HAP_MAX     8u
#define VC_POA_HAP_INDELS  1u      /* vc_poa_hap_params::flags: GAP is an allele                       */
#define VC_POA_HAP_NONE    0xFFu   /* hap_of of a member that was not added, or of a group not VC_WIN_OK */

typedef struct vc_poa_hap_params {
    uint32_t max_haplotypes;      /* 1 .. VC_POA_HAP_MAX, default 2 */
    uint32_t min_reads;           /* >= 1, default 2                */
    uint32_t min_permille;        /* 0 .. 1000, default 250         */
    uint32_t rounds;              /* >= 1, default 4                */
    uint32_t flags;               /* VC_POA_HAP_INDELS              */
} vc_poa_hap_params;

typedef struct vc_poa_hap_out {       /* library-owned, lifetime as vc_poa_msa_out */
    uint32_t        n_groups;
    const uint32_t* n_haps;       /* [n_groups]                                                           */
    const uint64_t* hap_first;    /* [n_groups + 1] first haplotype of the group                          */
    const uint32_t* hap_size;     /* [haplotypes] members                                                 */
    const uint64_t* cons_off;     /* [haplotypes + 1] into cons                                           */
    const uint8_t*  cons;
    const uint8_t*  hap_of;       /* [n_seqs of b] haplotype of the member within its group, or VC_POA_HAP_NONE */
    const uint64_t* site_off;     /* [n_groups + 1] into the site arrays                                  */
    const uint32_t* site_col;     /* column of the alignment                                              */
    const uint8_t*  site_major;   /* decoded byte, or '-'                                                 */
    const uint8_t*  site_minor;
    const uint32_t* site_n_major;
    const uint32_t* site_n_minor;
    uint64_t        bytes;        /* copied out of the device                                             */
} vc_poa_hap_out;

void        vc_poa_hap_default_params(vc_poa_hap_params* h);
int         vc_poa_run_haplotypes(const vc_poa_gap_params* p, const vc_poa_hap_params* h, const vc_batch* b, vc_result* r,
                                  vc_poa_hap_out* o);

/* ------------------------------------------------------------------------------------------------
 * All-vs-all read overlaps on the device (vechat_amd/csrc/vc_overlap.hip): the first step of both rounds, which the reference's
 * wrapper leaves to an external command (scripts/vechat:36-49).
 *
 * THIS IS THE LIBRARY'S OWN RULE.  It is written in the spirit of
 *     minimap2 -x ava-ont | awk '$11>=500' | fpa drop --same-name --internalmatch
 * (minimizer sketch, seeds by shared minimizer, colinear chaining, PAF records, internal matches dropped) and it is NOT a
 * byte-for-byte restatement of either tool: their heuristics (secondary chains, z-drop, homopolymer compression, occurrence
 * thresholds as fractions) are left out.  Everything below is integer arithmetic and every tie is decided, so the records are a
 * function of the input alone; tests/overlap_ref.py restates the rule on the CPU and the device is pinned to it array for array.
 *
 * Input: two sequence sets, targets and queries, each as offsets plus bases (any byte; only ACGTacgt make k-mers).  With same_set
 * the queries ARE the targets: `queries` is not read (it may be NULL), one table is sketched, and pair (i, i) is never produced --
 * pair (i, j) and pair (j, i) both are, as `--dual=yes` gives them.
 *
 * Sketch.  Bases are coded A 0, C 1, G 2, T 3 (either case).  The k-mer whose LAST base is position p exists when the k bases
 * p - k + 1 .. p are all ACGTacgt.  fw is its 2k-bit value, first base highest; rv is the value of its reverse complement.
 * fw == rv: the k-mer is skipped -- it holds its place in a window and can never be the minimum.  Otherwise strand = (rv < fw)
 * and hash = mix(min(fw, rv)), Wang's invertible mix on 2k bits, with mask = 2^(2k) - 1:
 *     x = (~x + (x << 21)) & mask;   x ^= x >> 24;   x = (x + (x << 3) + (x << 8)) & mask;   x ^= x >> 14;
 *     x = (x + (x << 2) + (x << 4)) & mask;   x ^= x >> 28;   x = (x + (x << 31)) & mask;
 * A window is w consecutive positions whose k-mers all exist (so no window contains or crosses a byte outside ACGTacgt, and a
 * stretch with fewer than w k-mers has none: a sequence shorter than k + w - 1 has no minimizer).  Position p is a minimizer
 * when its k-mer is not skipped and it is the leftmost minimum hash, over the k-mers not skipped, of at least one window.
 * vc_overlap_sketch returns the table (hash, seq, pos = p, strand) sorted by (seq, pos).  No homopolymer compression.
 *
 * Seeds.  The entries of both tables (of the one table with same_set) are sorted by hash.  A hash with more than max_occ
 * entries, counted over targets and queries together (over the one table with same_set), is dropped.  For every other hash,
 * every (target entry, query entry) gives an anchor -- with same_set: every ordered pair of entries of different sequences.
 * rel_strand = target strand ^ query strand.  The anchor's key is (t_id, q_id, rel_strand) and its positions are (t_pos, q_pos),
 * t_pos = the target entry's pos, q_pos = the query entry's pos for rel_strand 0 and q_len - pos + k - 2 for rel_strand 1: the
 * last base of the same k-mer on the reverse-complemented query.
 * The anchors of a call may not fit the device: the target range is cut into pieces of consecutive targets whose anchors fit
 * the budget (half of the free device memory; at least one target per piece) and run piece by piece.  Keys never span pieces,
 * so the records do not depend on the cut.
 *
 * Chain.  One problem per key.  Its anchors are sorted by (t_pos, q_pos) and numbered 0 .. n - 1.  With dt = t_pos(i) - t_pos(j),
 * dq = q_pos(i) - q_pos(j), d = |dt - dq|, anchor j is an admissible predecessor of i when i - lookback <= j < i,
 * 0 < dt <= max_gap, 0 < dq <= max_gap and d <= bandwidth; then
 *     gain(j, i) = min(dt, dq, k)        cost(j, i) = d == 0 ? 0 : (d * k) / 100 + ilog2(d) / 2        (integer divisions)
 *     v(i) = max over admissible j of f(j) + gain - cost, ties to the largest j
 *     f(i) = v(i), pred(i) = that j   when v(i) > k;        f(i) = k, pred(i) = none   otherwise.
 * The chain of the key ends at the anchor of maximum f, ties to the smallest i, and follows pred back.  score = that f,
 * n_anchors = its length; it is kept when score >= min_chain_score and n_anchors >= min_anchors.  One chain per key.
 *
 * Record.  With first / last the chain's first and last anchor: t_begin = t_pos(first) - k + 1, t_end = t_pos(last) + 1, and the
 * same on the query in its orientation, qb and qe; q_begin = qb, q_end = qe for strand 0 and q_begin = q_len - qe,
 * q_end = q_len - qb for strand 1 (PAF's forward coordinates).  block = max(q_end - q_begin, t_end - t_begin);
 * matches = k + the sum of gain along the chain.  A record with block < min_overlap is dropped.  With drop_internal, with
 * left = min(qb, t_begin) and right = min(q_len - qe, t_len - t_end) -- the shorter unanchored end on each side in the query's
 * orientation.  A chain ends at its outermost shared minimizer, not where the alignment ends: shared minimizers fall along an
 * overlap like a Poisson process of mean spacing block / n_anchors, so the alignment reaches a further spacing beyond the chain on
 * average and more than three spacings with probability e^-3 = 5 %.  Each end is therefore granted
 *     slack = (3 * block) / n_anchors                                                       (integer division)
 * and the overhangs and the aligned part are  l = max(left - slack, 0),  r = max(right - slack, 0),
 * aligned = block + (left - l) + (right - r).  A record is an internal match and dropped when
 *     l > 1000   or   r > 1000   or   5 * aligned < 4 * (aligned + l + r).
 * (At 6 % errors per read the slack is some 70 bases; at 10 % some 250, where the test on the bare chain ends took 134 of 214
 * chained true overlaps of 1.5 kb reads for internal matches.)
 * Containments are kept.  A record that passes this test is a dovetail or a containment up to its overhangs, and a chain ends
 * where the last shared minimizer happens to lie -- at 6 % errors per read often hundreds of bases short of the read end.  So,
 * with drop_internal only, the ends are then moved out along the chain's end diagonals to the nearer read end: qb and t_begin
 * decrease by left, qe and t_end increase by right (before the query is mapped to forward coordinates), and block is taken
 * again from the new ends; matches stays the chain's.  Without drop_internal the ends are the chain's.
 * The records are ordered by (q_id, t_id, strand), whatever the launch shape and the budget.
 *
 * Envelope: at most VC_OVL_MAX_SEQS sequences per set, each at most VC_OVL_MAX_LEN bases; max_occ <= VC_OVL_MAX_OCC; max_gap and
 * bandwidth <= VC_OVL_MAX_GAP; fewer than 2^31 minimizers per call and fewer than 2^31 anchors per target (VC_ERR_HIP with a
 * text, found on the device).
 * Checked on the host before the device is touched, in this order: p, targets, queries (without same_set), out NULL, or a set
 * without offsets; offsets that do not start at 0 or decrease, or bases missing beside a non-empty set; k outside 4..28; w outside
 * 1..64; lookback other than 64; a zero or negative max_occ, max_gap, bandwidth, min_chain_score, min_anchors or min_overlap, or
 * drop_internal / same_set other than 0 / 1; a limit, a sequence count or a length beyond the envelope: VC_ERR_ARG.
 * VC_ERR_NO_DEVICE only after these.  vc_overlap_sketch checks its own arguments in the same order.
 * Lifetime: the library owns every array of vc_overlap_out and vc_overlap_sketch_out -- one set each per process, not
 * thread-safe.  They stay valid until the next call of the same entry or vc_overlap_release; a failed call leaves every
 * pointer NULL.  vc_overlap_last_error has the text of the last failure.
 * Test knobs, read on every vc_overlap call: VC_OVL_BUDGET_MB=x (the budget of one piece in MiB, fractions allowed) and
 * VC_OVL_LOG (one stderr line per piece, "vc_overlap: piece first=T targets=N anchors=A keys=K records=R").
 * ------------------------------------------------------------------------------------------------ */
#define VC_OVL_MAX_SEQS 0x7FFFFFFFull
#define VC_OVL_MAX_LEN  0x40000000ull
#define VC_OVL_MAX_OCC  65536
#define VC_OVL_MAX_GAP  16777216
typedef struct vc_overlap_seqs {
    uint64_t        n;               /* sequences                          */
    const uint64_t* off;             /* [n + 1] into bases, off[0] == 0    */
    const uint8_t*  bases;
} vc_overlap_seqs;
typedef struct vc_overlap_params {   /* vc_overlap_default_params fills in the defaults named here                    */
    int32_t device;                  /* 0                                                                            */
    int32_t k;                       /* 15   (4..28)                                                                 */
    int32_t w;                       /* 5    (1..64)                                                                 */
    int32_t max_occ;                 /* 100                                                                          */
    int32_t max_gap;                 /* 5000                                                                         */
    int32_t bandwidth;               /* 500                                                                          */
    int32_t lookback;                /* 64: the only value accepted                                                  */
    int32_t min_chain_score;         /* 40                                                                           */
    int32_t min_anchors;             /* 3                                                                            */
    int32_t min_overlap;             /* 500                                                                          */
    int32_t drop_internal;           /* 1                                                                            */
    int32_t same_set;                /* 0; 1: the queries are the targets, pair (i, i) is never produced             */
} vc_overlap_params;
typedef struct vc_overlap_out {      /* library-owned; [n] each, ordered by (q_id, t_id, strand)                      */
    uint64_t        n;
    const uint32_t* q_id;
    const uint32_t* t_id;
    const uint8_t*  strand;          /* 1: the query is reverse-complemented                                         */
    const uint32_t* q_begin; const uint32_t* q_end;      /* forward coordinates, end exclusive                       */
    const uint32_t* t_begin; const uint32_t* t_end;
    const uint32_t* n_anchors;
    const int32_t*  score;
    const uint32_t* matches;         /* PAF column 10                                                                */
    const uint32_t* block;           /* PAF column 11                                                                */
    uint64_t n_minimizers, n_anchors_total, n_keys_total;     /* what the call went through                          */
} vc_overlap_out;
typedef struct vc_overlap_sketch_out {   /* library-owned; [n] each, sorted by (seq, pos)                             */
    uint64_t        n;
    const uint64_t* hash;
    const uint32_t* seq;
    const uint32_t* pos;             /* of the k-mer's last base                                                     */
    const uint8_t*  strand;          /* 1: the reverse complement is the smaller value                               */
} vc_overlap_sketch_out;
void        vc_overlap_default_params(vc_overlap_params* p);
int         vc_overlap(const vc_overlap_params* p, const vc_overlap_seqs* targets, const vc_overlap_seqs* queries /* not read with same_set */,
                       vc_overlap_out* out);
int         vc_overlap_sketch(int32_t device, int32_t k, int32_t w, const vc_overlap_seqs* s, vc_overlap_sketch_out* o);
const char* vc_overlap_last_error(void);
void        vc_overlap_release(void);

/* ------------------------------------------------------------------------------------------------
 * Scrubbing of chimeric reads on the device (vechat_amd/csrc/vc_scrub.hip): the step the reference's wrapper leaves to
 * `minimap2 -g ... | yacrd -c C -n F scrubb` (scripts/vechat:187-201).  A chimeric read joins two loci; no other read covers its
 * junction, so the junction shows as a stretch of low coverage strictly inside the read, and the read is cut there.
 *
 * THIS IS THE LIBRARY'S OWN RULE, in the spirit of `yacrd -c C -n F scrubb` (coverage from overlap intervals, badly covered
 * stretches, reads cut at them or dropped) and NOT a restatement of it.  Everything is integer arithmetic and every case is
 * decided; tests/scrub_ref.py restates the rule position by position and the device is pinned to it array for array.
 *
 * Input.  n reads with lengths len[r] (each at most VC_OVL_MAX_LEN, n at most VC_OVL_MAX_SEQS) and m intervals
 * (read, begin, end) with read < n and 0 <= begin < end <= len[read], in any order, 2 m < 2^31.  An interval says "another read
 * overlaps this stretch"; where intervals come from is the caller's business.  Optionally the bases of the reads as offsets plus
 * bytes (off[n + 1] with off[r + 1] - off[r] == len[r], and bases), and optionally their qualities, bytes under the same offsets.
 *
 * Coverage and bad regions.  cov_r(p) is the number of intervals of read r with begin <= p < end.  Position p is BAD when
 * cov_r(p) <= coverage (the threshold c).  The bad regions of a read are the maximal runs of bad positions, as [b, e).  A read
 * with no interval is one bad region [0, len).  A read of length 0 has no region.
 *
 * Class of a read.  bad_total is the sum of e - b over its regions.
 *     VC_SCRUB_NOT_COVERED 3   1000 * bad_total > max_bad_permille * len (in 64 bits); this is decided first
 *     VC_SCRUB_CHIMERIC    2   otherwise, some region has b > 0 and e < len
 *     VC_SCRUB_BAD_ENDS    1   otherwise, at least one region
 *     VC_SCRUB_CLEAN       0   otherwise
 *
 * Pieces.  A NOT_COVERED read has no pieces.  For every other read the pieces are the maximal runs of positions that are not
 * bad and whose length is at least min_piece, in order.
 *
 * Output, library-owned.  Regions (read, begin, end) ordered by (read, begin), with reg_off[n + 1] into them; per read klass and
 * bad_total; pieces (read, begin, end) ordered the same way, with pc_off[n_pieces + 1] into the cut bytes (filled in whether or
 * not bases were given).  With bases, pc_bases holds the bases of every piece back to back; with qualities, pc_quals the same of
 * the qualities.  Without, the pointer is NULL.  The result is a function of the input alone, not of the order of the intervals
 * and not of any launch shape.
 *
 * Checked on the host before the device is touched, in this order: p, in or out NULL, lengths NULL with n > 0, an interval array
 * NULL with m > 0, bases without offsets, qualities without bases; offsets that do not start at 0, decrease, or disagree with the
 * lengths; coverage outside 0..2^30, max_bad_permille outside 0..1000, min_piece below 1; an interval with read >= n, empty, or
 * ending beyond its read; n, a length or m beyond the envelope: VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these.  Device memory is
 * taken per call, with no piece-by-piece budget: a call whose buffers the device refuses is VC_ERR_HIP with a text.
 * Lifetime: the library owns every array of vc_scrub_out -- one set per process, not thread-safe -- until the next vc_scrub call
 * or vc_scrub_release; a failed call leaves every pointer NULL.  vc_scrub_last_error has the text of the last failure.
 * Test knob, read on every call: VC_SCRUB_LOG (one stderr line, "vc_scrub: intervals=M events=E segments=S regions=R pieces=P").
 * ------------------------------------------------------------------------------------------------ */
#define VC_SCRUB_CLEAN       0
#define VC_SCRUB_BAD_ENDS    1
#define VC_SCRUB_CHIMERIC    2
#define VC_SCRUB_NOT_COVERED 3
typedef struct vc_scrub_params {     /* vc_scrub_default_params fills in the defaults named here                      */
    int32_t device;                  /* 0                                                                            */
    int32_t coverage;                /* 0    the threshold c (0..2^30): a position covered c times or fewer is bad   */
    int32_t max_bad_permille;        /* 400  (0..1000)                                                               */
    int32_t min_piece;               /* 1    (at least 1)                                                            */
} vc_scrub_params;
typedef struct vc_scrub_in {
    uint64_t        n;               /* reads                                                                        */
    const uint32_t* len;             /* [n]                                                                          */
    uint64_t        m;               /* intervals                                                                    */
    const uint32_t* read;            /* [m]                                                                          */
    const uint32_t* begin;           /* [m]                                                                          */
    const uint32_t* end;             /* [m] exclusive                                                                */
    const uint64_t* off;             /* NULL, or [n + 1] into bases and quals                                        */
    const uint8_t*  bases;           /* NULL: nothing is cut                                                         */
    const uint8_t*  quals;           /* NULL: no qualities                                                           */
} vc_scrub_in;
typedef struct vc_scrub_out {        /* library-owned                                                                */
    uint64_t        n_regions;
    const uint32_t* reg_read;        /* [n_regions] ordered by (read, begin)                                         */
    const uint32_t* reg_begin;
    const uint32_t* reg_end;
    const uint64_t* reg_off;         /* [n + 1] the regions of read r are reg_off[r] .. reg_off[r + 1]               */
    const uint8_t*  klass;           /* [n] VC_SCRUB_*                                                               */
    const uint32_t* bad_total;       /* [n]                                                                          */
    uint64_t        n_pieces;
    const uint32_t* pc_read;         /* [n_pieces] ordered by (read, begin)                                          */
    const uint32_t* pc_begin;
    const uint32_t* pc_end;
    const uint64_t* pc_off;          /* [n_pieces + 1] into pc_bases / pc_quals                                      */
    const uint8_t*  pc_bases;        /* NULL without bases                                                           */
    const uint8_t*  pc_quals;        /* NULL without qualities                                                       */
    uint64_t n_intervals, n_events, n_segments;               /* what the call went through                          */
} vc_scrub_out;
void        vc_scrub_default_params(vc_scrub_params* p);
int         vc_scrub(const vc_scrub_params* p, const vc_scrub_in* in, vc_scrub_out* out);
const char* vc_scrub_last_error(void);
void        vc_scrub_release(void);

/* ------------------------------------------------------------------------------------------------
 * Clustering of reads into POA groups on the device (vechat_amd/csrc/vc_cluster.hip): overlaps go in, read groups come out --
 * the groups that vc_poa_run and its kin expect the caller to arrive with (UMI families, amplicon clusters, reads of one locus).
 *
 * THIS IS THE LIBRARY'S OWN RULE: single-linkage clustering on qualified overlaps, with the strand of every read worked out on
 * the way.  It restates no other tool.  Everything is integer arithmetic in 64 bits and every tie is decided;
 * tests/cluster_ref.py restates the rule with another algorithm and the device is pinned to it array for array.
 *
 * Input.  n reads with lengths len[r] and m overlap records with the fields of vc_overlap_out that matter here: q_id, t_id,
 * strand, q_begin, q_end, t_begin, t_end, matches, block.  The records may come in any order, with duplicates and with both
 * directions of a pair; where they come from is the caller's business, as for vc_scrub.
 *
 * Link.  A record links its two reads a = q_id and b = t_id when all of these hold:
 *     a != b
 *     block >= min_overlap
 *     1000 * matches >= min_identity_permille * block      (min_identity_permille == 0 switches this test off; matches is read
 *                                                           as given: the chain's figure, or the exact one if the caller aligned)
 *     the cover test: with  ca = 1000 * (q_end - q_begin) >= min_cover_permille * len[a]
 *                     and   cb = 1000 * (t_end - t_begin) >= min_cover_permille * len[b],
 *                     cover_both == 1 requires ca && cb (reads that overlap end to end, such as amplicons),
 *                     cover_both == 0 requires ca || cb (a short read contained in a long one).
 * Equality passes every threshold.
 *
 * Components with strands.  The graph has 2 n nodes, node 2 r + s for read r in orientation s.  A linking record with strand g
 * joins (2 a, 2 b + g) and (2 a + 1, 2 b + 1 - g).  label(v) is the smallest node of v's component.  Per read:
 *     root[r]    = label(2 r) >> 1                  the smallest read index of the cluster
 *     strand[r]  = label(2 r) & 1                   1: reverse-complement r to put it in the root's orientation
 *     twisted[r] = label(2 r) == label(2 r + 1)     the records contradict each other about the orientation; then strand is 0
 *                                                   for every read of the cluster
 * So every output is a function of the record SET alone: not of the record order, the launch shape or who wins an atomic.
 *
 * Clusters.  The reads with equal root form a cluster; a read without a link is a cluster of one.  A cluster with fewer than
 * min_size reads is dropped and its reads get cluster[r] = VC_CLUSTER_NONE.  Kept clusters are numbered from 0: with
 * by_size == 0 by root ascending, with by_size == 1 by size descending, ties by root ascending.  The members of a cluster are
 * ordered by read index ascending (longest_first == 0) or by len descending, ties by index ascending (longest_first == 1: the
 * longest read becomes the POA backbone).
 *
 * Output, library-owned.  cl_off[n_clusters + 1] into members; members[cl_off[n_clusters]], the read indices cluster by cluster;
 * cl_root[n_clusters]; cl_twisted[n_clusters]; per read cluster[n] and strand[n] (strand is given for dropped reads too).
 * Counters: n_links, the records that link (duplicates counted); n_rounds, the hook launches of the call (the components come
 * from one lock-free hook kernel: 1, or 0 when no record links); n_components, the clusters before min_size is applied.
 *
 * Envelope: n <= VC_CLUSTER_MAX_READS = 2^30 (2 n nodes fit 31 bits), m < 2^30, every length at most VC_OVL_MAX_LEN.
 * Checked on the host before the device is touched, in this order: p, in or out NULL, lengths NULL with n > 0, a record array
 * NULL with m > 0; min_overlap below 0, min_cover_permille outside 0..1000, cover_both other than 0 / 1, min_identity_permille
 * outside 0..1000, min_size below 1, by_size or longest_first other than 0 / 1; a record with q_id or t_id >= n, with an empty
 * interval, with an interval ending beyond its read, or with a strand other than 0 / 1; n, a length or m beyond the envelope:
 * VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these.  Device memory is taken per call: a call whose buffers the device refuses is
 * VC_ERR_HIP with a text.
 * Lifetime: the library owns every array of vc_cluster_out -- one set per process, not thread-safe -- until the next vc_cluster
 * call or vc_cluster_release; a failed call leaves every pointer NULL.  vc_cluster_last_error has the text of the last failure.
 * Test knob, read on every call: VC_CLUSTER_LOG (one stderr line, "vc_cluster: records=M links=L rounds=R components=C kept=K").
 * ------------------------------------------------------------------------------------------------ */
#define VC_CLUSTER_NONE      0xFFFFFFFFu
#define VC_CLUSTER_MAX_READS 0x40000000ull
typedef struct vc_cluster_params {   /* vc_cluster_default_params fills in the defaults named here                    */
    int32_t device;                  /* 0                                                                            */
    int32_t min_overlap;             /* 500  (at least 0)                                                            */
    int32_t min_cover_permille;      /* 800  (0..1000)                                                               */
    int32_t cover_both;              /* 1    0: one side of the record is enough                                     */
    int32_t min_identity_permille;   /* 0    (0..1000); 0: no identity test                                          */
    int32_t min_size;                /* 2    (at least 1)                                                            */
    int32_t by_size;                 /* 0    1: clusters numbered by size descending                                 */
    int32_t longest_first;           /* 0    1: members by length descending                                         */
} vc_cluster_params;
typedef struct vc_cluster_in {
    uint64_t        n;               /* reads                                                                        */
    const uint32_t* len;             /* [n]                                                                          */
    uint64_t        m;               /* records; [m] each of the nine arrays below                                   */
    const uint32_t* q_id;
    const uint32_t* t_id;
    const uint8_t*  strand;
    const uint32_t* q_begin; const uint32_t* q_end;
    const uint32_t* t_begin; const uint32_t* t_end;
    const uint32_t* matches;
    const uint32_t* block;
} vc_cluster_in;
typedef struct vc_cluster_out {      /* library-owned                                                                */
    uint64_t        n_clusters;
    const uint64_t* cl_off;          /* [n_clusters + 1] the members of cluster c are cl_off[c] .. cl_off[c + 1]     */
    const uint32_t* members;         /* [cl_off[n_clusters]] read indices                                            */
    const uint32_t* cl_root;         /* [n_clusters] the smallest read index of the cluster                          */
    const uint8_t*  cl_twisted;      /* [n_clusters] 1: the records contradict each other about the orientation      */
    const uint32_t* cluster;         /* [n] the cluster of read r, or VC_CLUSTER_NONE                                */
    const uint8_t*  strand;          /* [n] 1: reverse-complement r to put it in its root's orientation              */
    uint64_t n_links, n_rounds, n_components;                 /* what the call went through                          */
} vc_cluster_out;
void        vc_cluster_default_params(vc_cluster_params* p);
int         vc_cluster(const vc_cluster_params* p, const vc_cluster_in* in, vc_cluster_out* out);
const char* vc_cluster_last_error(void);
void        vc_cluster_release(void);

/* ------------------------------------------------------------------------------------------------
 * Demultiplexing, orienting and trimming of reads by adapter, primer and barcode on the device (vechat_amd/csrc/vc_demux.hip):
 * the step in front of the POA groups -- reads of several samples in one file, on both strands, each starting with a barcode
 * or primer and ending with the reverse complement of one -- that otherwise goes to cutadapt, porechop or minibar.
 *
 * THIS IS THE LIBRARY'S OWN RULE, in the spirit of cutadapt and minibar (approximate matching of short patterns near the read
 * ends) and a restatement of neither.  Nothing in the reference corresponds to it.  Everything is integer arithmetic and every
 * tie is decided; tests/demux_ref.py restates the rule with full tables and the device is pinned to it array for array.
 *
 * Input.  n reads as offsets plus bytes (off[n + 1], bases), optionally their qualities under the same offsets.  P patterns as
 * offsets plus bytes, pattern j of length m_j in 1..64, with label[j] < VC_DEMUX_MAX_LABELS (patterns of one label are one
 * sample, barcode or amplicon) and side[j] in VC_DEMUX_ANY / _HEAD / _TAIL.  A pattern byte is an upper-case IUPAC code
 * (ACGT RYSWKM BDHV N) and stands for its set of bases.  A read byte other than A C G T (N, lower case) matches no pattern byte.
 *
 * Views.  Every read has two views of length L = min(len, window).  View 0, the head, is read[0:L].  View 1, the tail, is the
 * first L bases of the read's reverse complement: view position p of the tail is read position len - 1 - p, complemented; the
 * complement of a byte outside ACGT is itself.  A barcode ligated to both ends, and the reverse primer of a + read, therefore
 * appear in the tail view as written 5'->3'.
 *
 * Hit of a (read, view, pattern) triple, pattern of length m:
 *     D[i][0] = i,  D[0][j] = 0,  D[i][j] = min(D[i-1][j-1] + mis, D[i-1][j] + 1, D[i][j-1] + 1),
 *     mis = 0 iff view[j-1] is in the set of pattern[i-1]
 *     d = min_j D[m][j];  e = the smallest j that attains d
 *     start: the same recurrence on the reversed pattern and reverse(view[0:e]), anchored with E[0][j] = j;
 *     k = the smallest j with E[m][j] == d;  s = e - k, the shortest hit that ends at e
 * An empty view gives d = m, s = e = 0.  The hit is ACCEPTED iff 1000 * d <= max_err_permille * m.
 *
 * Per (read, view).  Accepted hits are ranked by smaller d, then larger m, then smaller j.  The best gives v_pat, v_dist,
 * v_start, v_end.  v_second is the d of the best-ranked accepted hit whose label differs from the best's, 255 if there is none.
 * The view is NONE when nothing is accepted (v_pat = VC_DEMUX_UNASSIGNED, v_dist = 255, v_start = v_end = 0, v_second = 255),
 * AMBIG when v_second != 255 and v_second - v_dist < min_margin, and otherwise its best hit's label.
 *
 * Per read.  plus holds when the head view is a label whose best pattern has side HEAD or the tail view is a label whose best
 * pattern has side TAIL; minus holds when the head's has side TAIL or the tail's has side HEAD.  The class, decided in this order:
 *     1 both views NONE                                              VC_DEMUX_NONE 0
 *     2 plus && minus, or both views are labels and differ            VC_DEMUX_CONFLICT 3
 *     3 both views are the same label                                VC_DEMUX_BOTH_ENDS 2, that label
 *     4 one view is a label and the other NONE                       VC_DEMUX_ONE_END 1, that label; with VC_DEMUX_REQUIRE_BOTH
 *                                                                    the label is VC_DEMUX_UNASSIGNED
 *     5 anything else                                                VC_DEMUX_AMBIGUOUS 4
 * Classes 0, 3 and 4 have label VC_DEMUX_UNASSIGNED.  flip = minus && !plus; it is reported in every case and applied to the cut
 * bytes only with VC_DEMUX_ORIENT.  The kept range [begin, end) is in read coordinates and comes from the views' best accepted
 * hits whatever the class: begin = v_end(head) with trim 1, v_start(head) with trim 2, 0 with trim 0 or a NONE head;
 * end = len - v_end(tail) with trim 1, len - v_start(tail) with trim 2, len with trim 0 or a NONE tail; begin >= end gives the
 * empty piece end = begin.
 *
 * Output, library-owned.  The per-view arrays [2 n] at index 2 r + view; per read klass, label, flip, begin, end;
 * piece_off[n + 1] into pc_bases and pc_quals, the kept bytes of every read back to back (with VC_DEMUX_ORIENT and flip
 * reverse-complemented, the qualities reversed), NULL without the input; groups grp_off[n_labels + 1] into grp_reads, the reads
 * with a label ordered by (label, read), n_labels = 1 + the largest label[j] (0 without patterns); with VC_DEMUX_ALL_HITS
 * all_dist and all_end, [2 n P] at index (2 r + view) * P + j, else NULL; and the counts the call went through.  The result is
 * a function of the input alone, not of any launch shape and not of how the reads are cut into pieces of the budget.
 *
 * The [2 n P] table of the search is produced per piece of consecutive reads; a piece's table fits the budget of
 * VC_DEMUX_BUDGET_MB MiB (a test knob, fractions allowed; 256 when unset), one read at least.
 * Envelope: n <= VC_OVL_MAX_SEQS, every read at most VC_OVL_MAX_LEN bases, P <= VC_DEMUX_MAX_PATTERNS.
 * Checked on the host before the device is touched, in this order: p, in or out NULL, read offsets or bases NULL with
 * n > 0, one of the four pattern arrays NULL with P > 0; read offsets, then pattern offsets, that do not start at 0 or decrease; window outside
 * 1..4096, max_err_permille outside 0..1000, min_margin outside 0..64, trim outside 0..2, flag bits other than the three;
 * P == 0 with n > 0; a pattern of length 0 or above 64, a pattern byte that is no IUPAC code, a side above 2, a label of
 * VC_DEMUX_MAX_LABELS or more; n, a read length or P beyond the envelope: VC_ERR_ARG.  VC_ERR_NO_DEVICE only after these.
 * Lifetime: the library owns every array of vc_demux_out -- one set per process, not thread-safe -- until the next vc_demux call
 * or vc_demux_release; a failed call leaves every pointer NULL.  vc_demux_last_error has the text of the last failure.
 * Test knob, read on every call: VC_DEMUX_LOG (one stderr line, "vc_demux: reads=N triples=T pieces=K accepted=A").
 * ------------------------------------------------------------------------------------------------ */
#define VC_DEMUX_ANY  0
#define VC_DEMUX_HEAD 1
#define VC_DEMUX_TAIL 2
#define VC_DEMUX_NONE       0
#define VC_DEMUX_ONE_END    1
#define VC_DEMUX_BOTH_ENDS  2
#define VC_DEMUX_CONFLICT   3
#define VC_DEMUX_AMBIGUOUS  4
#define VC_DEMUX_REQUIRE_BOTH 1
#define VC_DEMUX_ORIENT       2
#define VC_DEMUX_ALL_HITS     4
#define VC_DEMUX_UNASSIGNED   0xFFFFFFFFu
#define VC_DEMUX_MAX_LABELS   0x100000u
#define VC_DEMUX_MAX_PATTERNS 65536
typedef struct vc_demux_params {     /* vc_demux_default_params fills in the defaults named here                      */
    int32_t device;                  /* 0                                                                            */
    int32_t window;                  /* 150  (1..4096) bases of each read end that are searched                      */
    int32_t max_err_permille;        /* 200  (0..1000)                                                               */
    int32_t min_margin;              /* 2    (0..64)                                                                 */
    int32_t trim;                    /* 1    0 keep everything, 1 cut the pattern and what lies outside it,          */
                                     /*      2 keep the pattern and cut outside it                                   */
    int32_t flags;                   /* 0    VC_DEMUX_REQUIRE_BOTH | VC_DEMUX_ORIENT | VC_DEMUX_ALL_HITS             */
} vc_demux_params;
typedef struct vc_demux_in {
    uint64_t        n;               /* reads                                                                        */
    const uint64_t* off;             /* [n + 1] into bases and quals                                                 */
    const uint8_t*  bases;
    const uint8_t*  quals;           /* NULL: no qualities                                                           */
    uint64_t        n_patterns;      /* P                                                                            */
    const uint64_t* pat_off;         /* [P + 1] into pat_bases                                                       */
    const uint8_t*  pat_bases;       /* upper-case IUPAC codes                                                       */
    const uint32_t* label;           /* [P]                                                                          */
    const uint8_t*  side;            /* [P] VC_DEMUX_ANY / _HEAD / _TAIL                                             */
} vc_demux_in;
typedef struct vc_demux_out {        /* library-owned                                                                */
    const uint32_t* v_pat;           /* [2 n] the best accepted pattern of the view, or VC_DEMUX_UNASSIGNED          */
    const uint8_t*  v_dist;          /* [2 n] its distance, or 255                                                   */
    const uint32_t* v_start;         /* [2 n] view coordinates                                                       */
    const uint32_t* v_end;           /* [2 n] exclusive                                                              */
    const uint8_t*  v_second;        /* [2 n] or 255                                                                 */
    const uint8_t*  klass;           /* [n] VC_DEMUX_NONE .. VC_DEMUX_AMBIGUOUS                                      */
    const uint32_t* label;           /* [n] or VC_DEMUX_UNASSIGNED                                                   */
    const uint8_t*  flip;            /* [n]                                                                          */
    const uint32_t* begin;           /* [n] read coordinates                                                         */
    const uint32_t* end;             /* [n] exclusive                                                                */
    const uint64_t* piece_off;       /* [n + 1] into pc_bases / pc_quals                                             */
    const uint8_t*  pc_bases;        /* NULL without bases (n == 0)                                                  */
    const uint8_t*  pc_quals;        /* NULL without qualities                                                       */
    uint64_t        n_labels;
    const uint64_t* grp_off;         /* [n_labels + 1] the reads of label g are grp_off[g] .. grp_off[g + 1]         */
    const uint32_t* grp_reads;       /* [grp_off[n_labels]] ordered by (label, read)                                 */
    const uint8_t*  all_dist;        /* NULL, or [2 n P] with VC_DEMUX_ALL_HITS                                      */
    const uint32_t* all_end;         /* NULL, or [2 n P]                                                             */
    uint64_t n_reads, n_triples, n_budget_pieces, n_accepted; /* what the call went through                          */
} vc_demux_out;
void        vc_demux_default_params(vc_demux_params* p);
int         vc_demux(const vc_demux_params* p, const vc_demux_in* in, vc_demux_out* out);
const char* vc_demux_last_error(void);
void        vc_demux_release(void);

#ifdef __cplusplus
}
#endif
#endif
