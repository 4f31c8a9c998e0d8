// Demultiplexing, orienting and trimming of reads by adapter, primer and barcode on the device: the step in front of the POA
// groups that otherwise goes to cutadapt, porechop or minibar.  Reads and patterns go in; per read end the best pattern with its
// distance and place, per read a class, a label, a strand and the kept range, the kept bytes and the reads of every label come back.
//
// Nothing in the reference corresponds to this step, so, like vc_overlap.hip, vc_scrub.hip and vc_cluster.hip, the library fixes
// its OWN rule -- all integer, every tie decided, written out in include/vechat_hip.h -- and tests/demux_ref.py restates it with
// full dynamic-programming tables, without a bit vector and without sharing a line with this file; tests/test_demux_gpu.py compares
// the two array for array.
//
// Test knobs, read with getenv on every call:
//   VC_DEMUX_BUDGET_MB   MiB (fractions allowed) of the [2 n P] search table held at a time; the reads are taken in pieces of
//                        consecutive reads whose table fits it (one read at least); 256 when unset
//   VC_DEMUX_LOG         set: one line per call on stderr, "vc_demux: reads=N triples=T pieces=K accepted=A"
//
// Kernels (gfx950, wave64):
//   k_dmx_masks     one lane per pattern: the four match masks of the pattern (bit i of mask b: base b is in the set of pattern
//                   byte i) and of the reversed pattern, the IUPAC sets already in them
//   k_dmx_search    the hot one.  One lane per (read, view, pattern) triple, view-major, so consecutive lanes are the patterns of
//                   one view: they read the same LDS address (a broadcast) and run the same number of steps.  Myers' bit-vector
//                   recurrence on one 64-bit column state, the four masks in registers.  The block stages kChunk characters of
//                   each of its views at a time in LDS -- as codes 0..3, 4 for a byte that matches nothing, the tail view read
//                   backwards and complemented --, a row per view with an odd stride in dwords, and a lane takes four characters
//                   with one ds_read_b32.  The 64-bit add of the recurrence is written as one: the compiler makes the carry pair.
//                   The state needs no masking beyond the start: bits at and above m never reach the bits below (carries and
//                   shifts only go up), and the score reads bit m - 1 alone, so m = 64 is not special.  A lane runs whole words:
//                   the up to three characters past the view's end are code 4, and a column of mismatches never lowers the last
//                   row (D[i][j] >= D[i][j-1] for such a column), so the first minimum stays where it was.
//   k_dmx_pick      one lane per (read, view) over its P results: acceptance, rank, the second label; then the anchored pass on
//                   the reversed pattern backwards from the end of the best hit, until the distance is met: its start
//   k_dmx_classify  one lane per read: class, label, flip and the kept range; the piece length for the scan and the label as sort key
//   k_dmx_first     one lane per label: where its reads begin in the sorted keys
//   k_dmx_cut       the one bandwidth kernel, in the manner of k_scr_cut: one thread per 16 output bytes, bases and qualities in one
//                   launch; a flipped piece is read backwards, 16 bytes at a time, and complemented in registers
//
// Host: vc_demux() is the argument checks, the uploads, one search and pick launch per piece of the budget (no launch per pattern,
// no loop over reads), and then classify, the scan of the piece lengths, the sort by (label, read) and the cut, once each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vechat_hip.h"

#include "vc_devscan.h"

namespace {

using namespace vc_dev;

constexpr uint32_t kNoDist = 255;
constexpr int kChunk = 64;                     // characters of a view staged at a time
constexpr int kRowWords = kChunk / 4 + 1;      // dwords of a row: odd, so that the rows of a wave fall on different banks
constexpr int kRows = 256;                     // views of a block at most (P == 1; 129 from P == 2 on)
constexpr uint32_t kLabelBits = 21;            // the sort key: a label below 2^20, or 2^20 for a read without one

// bit b of the result: base b of ACGT is in the set of the IUPAC code c; 0: c is no code
__host__ __device__ inline uint32_t iupac_set(uint8_t c) {
    switch (c) {
        case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
        case 'R': return 5; case 'Y': return 10; case 'S': return 6; case 'W': return 9; case 'K': return 12; case 'M': return 3;
        case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
        default: return 0;
    }
}
__device__ __forceinline__ uint32_t code_of(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ uint8_t complement(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

__global__ void k_dmx_masks(uint32_t P, const uint64_t* pat_off, const uint8_t* pat, uint64_t* peq, uint64_t* rpeq, uint8_t* plen) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P) return;
    const uint64_t o = pat_off[j];
    const uint32_t m = (uint32_t)(pat_off[j + 1] - o);
    uint64_t f[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t set = iupac_set(pat[o + i]);
        for (int b = 0; b < 4; ++b)
            if (set >> b & 1) { f[b] |= 1ull << i; r[b] |= 1ull << (m - 1 - i); }
    }
    for (int b = 0; b < 4; ++b) { peq[4ull * j + b] = f[b]; rpeq[4ull * j + b] = r[b]; }
    plen[j] = (uint8_t)m;
}

// One column of Myers' recurrence (Hyyro's form).  anchored: the top row counts up (E[0][j] = j), else it is 0.
template <bool Anchored>
__device__ __forceinline__ void myers_step(uint64_t eq, uint64_t hi, uint64_t& pv, uint64_t& mv, uint32_t& score) {
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    score += (ph & hi) != 0;
    score -= (mh & hi) != 0;
    ph = ph << 1 | (Anchored ? 1u : 0u);
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

struct SearchArgs {
    uint64_t n_triples;                        // of the piece: its views times P
    uint64_t view0;                            // the first (read, view) of the piece, 2 * its first read
    uint32_t P, window;
    const uint64_t* off; const uint8_t* bases; // the read image
    const uint64_t* peq; const uint8_t* plen;
    uint32_t* res;                             // [n_triples] d << 16 | e
    uint8_t* all_dist; uint32_t* all_end;      // NULL, or [n_triples]
};

__global__ __launch_bounds__(256) void k_dmx_search(SearchArgs a) {
    __shared__ uint32_t tile[kRows * kRowWords];
    __shared__ uint64_t row_src[kRows];        // the byte of view position 0
    __shared__ uint32_t row_len[kRows];        // L, bit 31: the tail view
    __shared__ uint32_t max_len;
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * 256, t = t0 + tid;
    const uint64_t t_last = min(t0 + 255, a.n_triples - 1);
    const uint64_t v0 = t0 / a.P;
    const uint32_t n_rows = (uint32_t)(t_last / a.P - v0) + 1;
    if (tid == 0) max_len = 0;
    __syncthreads();
    if (tid < n_rows) {
        const uint64_t gv = a.view0 + v0 + tid, r = gv >> 1;
        const uint64_t o = a.off[r], len = a.off[r + 1] - o;
        const uint32_t L = (uint32_t)min<uint64_t>(len, a.window);
        const bool tail = gv & 1;
        row_src[tid] = tail ? o + len - 1 : o;             // (never read when L == 0)
        row_len[tid] = L | (tail ? 0x80000000u : 0u);
        atomicMax(&max_len, L);
    }
    const bool valid = t < a.n_triples;
    const uint32_t row = valid ? (uint32_t)(t / a.P - v0) : 0;
    const uint32_t j = valid ? (uint32_t)(t % a.P) : 0;
    const uint64_t pA = a.peq[4ull * j], pC = a.peq[4ull * j + 1], pG = a.peq[4ull * j + 2], pT = a.peq[4ull * j + 3];
    const uint32_t m = a.plen[j];
    const uint64_t hi = 1ull << (m - 1);
    uint64_t pv = m == 64 ? ~0ull : (1ull << m) - 1, mv = 0;
    uint32_t score = m, best = m, e = 0;
    __syncthreads();
    const uint32_t L = valid ? row_len[row] & 0x7FFFFFFFu : 0;
    const uint32_t longest = max_len;
    for (uint32_t c0 = 0; c0 < longest; c0 += kChunk) {
        for (uint32_t idx = tid; idx < n_rows * (kChunk / 4); idx += 256) {
            const uint32_t rw = idx / (kChunk / 4), w = idx % (kChunk / 4);
            const uint32_t rl = row_len[rw], len = rl & 0x7FFFFFFFu;
            const uint64_t src = row_src[rw];
            uint32_t word = 0;
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t p = c0 + 4 * w + b;
                uint32_t code = 4;
                if (p < len) code = rl >> 31 ? code_of(complement(a.bases[src - p])) : code_of(a.bases[src + p]);
                word |= code << (8 * b);
            }
            tile[rw * kRowWords + w] = word;
        }
        __syncthreads();
        const uint32_t n_words = L > c0 ? (min(L - c0, (uint32_t)kChunk) + 3) / 4 : 0;
        for (uint32_t w = 0; w < n_words; ++w) {
            const uint32_t word = tile[row * kRowWords + w];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t c = word >> (8 * b) & 0xFF;
                const uint64_t eq = c == 0 ? pA : c == 1 ? pC : c == 2 ? pG : c == 3 ? pT : 0ull;
                myers_step<false>(eq, hi, pv, mv, score);
                if (score < best) { best = score; e = c0 + 4 * w + b + 1; }
            }
        }
        __syncthreads();
    }
    if (!valid) return;
    a.res[t] = best << 16 | e;
    if (a.all_dist) { a.all_dist[t] = (uint8_t)best; a.all_end[t] = e; }
}

struct PickArgs {
    uint64_t n_views, view0;                   // the views of the piece, and its first one
    uint32_t P, permille;
    const uint32_t* res;                       // [n_views * P]
    const uint64_t* off; const uint8_t* bases;
    const uint64_t* rpeq; const uint8_t* plen; const uint32_t* label;
    uint32_t* v_pat; uint8_t* v_dist; uint32_t* v_start; uint32_t* v_end; uint8_t* v_second;      // [2 n], the whole call
    unsigned long long* accepted;
};

__global__ void k_dmx_pick(PickArgs a) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_views) return;
    const uint64_t gv = a.view0 + v;
    const uint32_t* res = a.res + v * a.P;
    uint32_t bd = kNoDist, bm = 0, bj = VC_DEMUX_UNASSIGNED, be = 0, n_acc = 0;
    for (uint32_t j = 0; j < a.P; ++j) {                     // ascending j: an equal (d, m) later does not replace
        const uint32_t d = res[j] >> 16, m = a.plen[j];
        if (1000u * d > a.permille * m) continue;
        ++n_acc;
        if (d < bd || (d == bd && m > bm)) { bd = d; bm = m; bj = j; be = res[j] & 0xFFFFu; }
    }
    if (n_acc) atomicAdd(a.accepted, (unsigned long long)n_acc);
    if (bj == VC_DEMUX_UNASSIGNED) {
        a.v_pat[gv] = VC_DEMUX_UNASSIGNED; a.v_dist[gv] = (uint8_t)kNoDist; a.v_start[gv] = 0; a.v_end[gv] = 0; a.v_second[gv] = (uint8_t)kNoDist;
        return;
    }
    const uint32_t lab = a.label[bj];
    uint32_t second = kNoDist;
    for (uint32_t j = 0; j < a.P; ++j) {
        const uint32_t d = res[j] >> 16;
        if (1000u * d <= a.permille * a.plen[j] && a.label[j] != lab) second = min(second, d);
    }
    // the start: the reversed pattern against view[e-1], view[e-2], ..., anchored; the first column at which the distance is met
    const uint64_t r = gv >> 1, o = a.off[r], len = a.off[r + 1] - o;
    const bool tail = gv & 1;
    const uint64_t* rp = a.rpeq + 4ull * bj;
    const uint64_t hi = 1ull << (bm - 1);
    uint64_t pv = bm == 64 ? ~0ull : (1ull << bm) - 1, mv = 0;
    uint32_t score = bm, k = 0;
    while (score != bd && k < be) {
        const uint32_t p = be - 1 - k;                       // view position
        const uint8_t byte = tail ? complement(a.bases[o + len - 1 - p]) : a.bases[o + p];
        const uint32_t c = code_of(byte);
        myers_step<true>(c < 4 ? rp[c] : 0ull, hi, pv, mv, score);
        ++k;
    }
    a.v_pat[gv] = bj; a.v_dist[gv] = (uint8_t)bd; a.v_start[gv] = be - k; a.v_end[gv] = be; a.v_second[gv] = (uint8_t)second;
}

struct ClassArgs {
    uint64_t n; uint32_t min_margin, trim, require_both;
    const uint64_t* off; const uint32_t* plabel; const uint8_t* pside;
    const uint32_t* v_pat; const uint8_t* v_dist; const uint32_t* v_start; const uint32_t* v_end; const uint8_t* v_second;
    uint8_t* klass; uint32_t* label; uint8_t* flip; uint32_t* begin; uint32_t* end;
    uint64_t* pc_len;                          // [n + 1], a 0 at the end
    uint32_t* key; uint32_t* val;              // [n] the label (2^20 without one) and the read
};

__global__ void k_dmx_classify(ClassArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n) return;
    constexpr uint32_t kNone = 0xFFFFFFFFu, kAmbig = 0xFFFFFFFEu;        // the states of a view that are no label
    uint32_t state[2], side[2];
    for (int v = 0; v < 2; ++v) {
        const uint32_t pat = a.v_pat[2 * r + v], d = a.v_dist[2 * r + v], second = a.v_second[2 * r + v];
        state[v] = pat == VC_DEMUX_UNASSIGNED ? kNone : (second != kNoDist && second - d < a.min_margin) ? kAmbig : a.plabel[pat];
        side[v] = state[v] < kAmbig ? a.pside[pat] : (uint32_t)VC_DEMUX_ANY;
    }
    const bool lab0 = state[0] < kAmbig, lab1 = state[1] < kAmbig;
    const bool plus = side[0] == VC_DEMUX_HEAD || side[1] == VC_DEMUX_TAIL;
    const bool minus = side[0] == VC_DEMUX_TAIL || side[1] == VC_DEMUX_HEAD;
    uint32_t klass, label = VC_DEMUX_UNASSIGNED;
    if (state[0] == kNone && state[1] == kNone) klass = VC_DEMUX_NONE;
    else if ((plus && minus) || (lab0 && lab1 && state[0] != state[1])) klass = VC_DEMUX_CONFLICT;
    else if (lab0 && lab1) { klass = VC_DEMUX_BOTH_ENDS; label = state[0]; }
    else if ((lab0 && state[1] == kNone) || (lab1 && state[0] == kNone)) { klass = VC_DEMUX_ONE_END; if (!a.require_both) label = lab0 ? state[0] : state[1]; }
    else klass = VC_DEMUX_AMBIGUOUS;
    const uint32_t len = (uint32_t)(a.off[r + 1] - a.off[r]);
    uint32_t b = 0, e = len;
    if (a.trim && a.v_pat[2 * r] != VC_DEMUX_UNASSIGNED) b = a.trim == 1 ? a.v_end[2 * r] : a.v_start[2 * r];
    if (a.trim && a.v_pat[2 * r + 1] != VC_DEMUX_UNASSIGNED) e = len - (a.trim == 1 ? a.v_end[2 * r + 1] : a.v_start[2 * r + 1]);
    if (b >= e) e = b;
    a.klass[r] = (uint8_t)klass; a.label[r] = label; a.flip[r] = (uint8_t)(minus && !plus); a.begin[r] = b; a.end[r] = e;
    a.pc_len[r] = e - b;
    if (r == 0) a.pc_len[a.n] = 0;
    a.key[r] = label == VC_DEMUX_UNASSIGNED ? VC_DEMUX_MAX_LABELS : label;
    a.val[r] = (uint32_t)r;
}

// grp_off[g], g = 0 .. n_labels: the first sorted read whose key is >= g
__global__ void k_dmx_first(uint32_t n_labels, uint64_t n, const uint32_t* key, uint64_t* grp_off) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_labels) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < g) lo = mid + 1; else hi = mid;
    }
    grp_off[g] = lo;
}

struct CutArgs {
    uint64_t total, n;                         // bytes of all pieces (> 0); reads
    uint32_t orient;
    const uint64_t* piece_off; const uint32_t* begin; const uint8_t* flip;
    const uint64_t* off;                       // [n + 1] the reads in the image
    const uint8_t* bases; const uint8_t* quals;            // the image (16 bytes of padding behind it); quals may be NULL
    uint8_t* out_bases; uint8_t* out_quals;
};

// 16 bytes from any address, as k_scr_cut takes them: one 16-byte load where the address allows it, else the five aligned words
// around them, shifted (the fifth at most 3 bytes past the 16, inside the padding at worst)
__device__ __forceinline__ uint4 dmx_load16(const uint8_t* base, uint64_t s) {
    if ((s & 15) == 0) return *reinterpret_cast<const uint4*>(base + s);
    const uint32_t sh = (uint32_t)(s & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (s - sh));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                      __builtin_amdgcn_alignbyte(w4, w3, sh));
}
__device__ __forceinline__ uint32_t complement4(uint32_t w) {
    return (uint32_t)complement((uint8_t)w) | (uint32_t)complement((uint8_t)(w >> 8)) << 8 | (uint32_t)complement((uint8_t)(w >> 16)) << 16 |
           (uint32_t)complement((uint8_t)(w >> 24)) << 24;
}
// the 16 bytes in the opposite order
__device__ __forceinline__ uint4 reverse16(uint4 x) {
    return make_uint4(__builtin_bswap32(x.w), __builtin_bswap32(x.z), __builtin_bswap32(x.y), __builtin_bswap32(x.x));
}

__global__ __launch_bounds__(256) void k_dmx_cut(CutArgs a) {
    const uint64_t n_chunks = (a.total + 15) / 16;
    for (uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < n_chunks; ch += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = ch * 16, o1 = min(o0 + 16, a.total);
        uint64_t lo = 0, hi = a.n;                           // the read of byte o0: the last one whose piece starts at or before it
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.piece_off[mid] <= o0) lo = mid; else hi = mid;
        }
        uint64_t r = lo;
        if (a.piece_off[r + 1] >= o0 + 16) {                 // the whole chunk lies in one piece: one aligned 16-byte store
            const uint64_t q0 = o0 - a.piece_off[r], src = a.off[r] + a.begin[r];
            if (a.orient && a.flip[r]) {
                const uint64_t s = src + (a.piece_off[r + 1] - a.piece_off[r]) - 16 - q0;
                uint4 x = reverse16(dmx_load16(a.bases, s));
                reinterpret_cast<uint4*>(a.out_bases)[ch] = make_uint4(complement4(x.x), complement4(x.y), complement4(x.z), complement4(x.w));
                if (a.quals) reinterpret_cast<uint4*>(a.out_quals)[ch] = reverse16(dmx_load16(a.quals, s));
            } else {
                reinterpret_cast<uint4*>(a.out_bases)[ch] = dmx_load16(a.bases, src + q0);
                if (a.quals) reinterpret_cast<uint4*>(a.out_quals)[ch] = dmx_load16(a.quals, src + q0);
            }
            continue;
        }
        for (uint64_t o = o0; o < o1; ++o) {                 // the tail of a piece and the heads of the next: byte by byte
            while (o >= a.piece_off[r + 1]) ++r;
            const uint64_t q = o - a.piece_off[r], src = a.off[r] + a.begin[r];
            if (a.orient && a.flip[r]) {
                const uint64_t s = src + (a.piece_off[r + 1] - a.piece_off[r]) - 1 - q;
                a.out_bases[o] = complement(a.bases[s]);
                if (a.quals) a.out_quals[o] = a.quals[s];
            } else {
                a.out_bases[o] = a.bases[src + q];
                if (a.quals) a.out_quals[o] = a.quals[src + q];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// what the library owns between calls (one set per process, like the vc_scrub_out arrays)
struct Owned {
    std::vector<uint32_t> v_pat, v_start, v_end, label, begin, end, grp_reads, all_end;
    std::vector<uint8_t> v_dist, v_second, klass, flip, pc_bases, pc_quals, all_dist;
    std::vector<uint64_t> piece_off, grp_off;
};
Owned g_own;

const char* check_offsets(uint64_t n, const uint64_t* off, const char* first, const char* order) {
    if (n == 0) return nullptr;
    if (off[0] != 0) return first;
    for (uint64_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return order;
    return nullptr;
}

const char* check_args(const vc_demux_params* p, const vc_demux_in* in) {
    const uint64_t n = in->n, P = in->n_patterns;
    if (n && (!in->off || !in->bases)) return "NULL argument: reads without offsets or bases";
    if (P && (!in->pat_off || !in->pat_bases || !in->label || !in->side)) return "NULL argument: patterns without an array";
    if (const char* e = check_offsets(n, in->off, "read offsets do not start at 0", "read offsets decrease")) return e;
    if (const char* e = check_offsets(P, in->pat_off, "pattern offsets do not start at 0", "pattern offsets decrease")) return e;
    if (p->window < 1 || p->window > 4096) return "window outside 1..4096";
    if (p->max_err_permille < 0 || p->max_err_permille > 1000) return "max_err_permille outside 0..1000";
    if (p->min_margin < 0 || p->min_margin > 64) return "min_margin outside 0..64";
    if (p->trim < 0 || p->trim > 2) return "trim outside 0..2";
    if (p->flags & ~(VC_DEMUX_REQUIRE_BOTH | VC_DEMUX_ORIENT | VC_DEMUX_ALL_HITS)) return "flags with a bit that is none of the three";
    if (P == 0 && n > 0) return "reads without a pattern";
    for (uint64_t j = 0; j < P; ++j) {
        const uint64_t m = in->pat_off[j + 1] - in->pat_off[j];
        if (m < 1 || m > 64) return "a pattern whose length is outside 1..64";
        for (uint64_t i = in->pat_off[j]; i < in->pat_off[j + 1]; ++i) if (!iupac_set(in->pat_bases[i])) return "a pattern byte that is no upper-case IUPAC code";
        if (in->side[j] > VC_DEMUX_TAIL) return "a side above 2";
        if (in->label[j] >= VC_DEMUX_MAX_LABELS) return "a label beyond the limit (VC_DEMUX_MAX_LABELS)";
    }
    if (n > VC_OVL_MAX_SEQS) return "more reads than the envelope (VC_OVL_MAX_SEQS)";
    for (uint64_t r = 0; r < n; ++r) if (in->off[r + 1] - in->off[r] > VC_OVL_MAX_LEN) return "a read longer than the envelope (VC_OVL_MAX_LEN)";
    if (P > VC_DEMUX_MAX_PATTERNS) return "more patterns than the envelope (VC_DEMUX_MAX_PATTERNS)";
    return nullptr;
}

// the device arrays of the whole call, and its counts
struct Dmx {
    uint64_t n = 0, P = 0, n_bytes = 0, n_budget_pieces = 0, total = 0;
    unsigned long long accepted = 0;
    uint32_t n_labels = 0;
    uint64_t *off = nullptr, *peq = nullptr, *rpeq = nullptr;
    uint8_t *bases = nullptr, *plen = nullptr, *pside = nullptr;
    uint32_t* plabel = nullptr;
    uint32_t *v_pat = nullptr, *v_start = nullptr, *v_end = nullptr;
    uint8_t *v_dist = nullptr, *v_second = nullptr;
    uint32_t *begin = nullptr; uint8_t* flip = nullptr; uint64_t* piece_off = nullptr;
};

// stage 1: the reads and the patterns on the device, the masks
int dmx_upload(DevMem& dm, const vc_demux_in* in, Dmx& s) {
    uint64_t* pat_off = nullptr; uint8_t* pat = nullptr;
    if (!dm.alloc(&s.off, s.n + 1, in->off) || !dm.alloc(&s.bases, s.n_bytes + 16) || !to_device(s.bases, in->bases, s.n_bytes))
        return fail(VC_ERR_HIP, "hipMalloc or upload failed (the read image)");
    if (!dm.alloc(&pat_off, s.P + 1, in->pat_off) || !dm.alloc(&pat, in->pat_off[s.P], in->pat_bases) || !dm.alloc(&s.plabel, s.P, in->label) ||
        !dm.alloc(&s.pside, s.P, in->side) || !dm.alloc(&s.peq, 4 * s.P) || !dm.alloc(&s.rpeq, 4 * s.P) || !dm.alloc(&s.plen, s.P))
        return fail(VC_ERR_HIP, "hipMalloc or upload failed (the patterns)");
    hipLaunchKernelGGL(k_dmx_masks, dim3(grid(s.P)), dim3(256), 0, 0, (uint32_t)s.P, pat_off, pat, s.peq, s.rpeq, s.plen);
    if (!ran()) return fail(VC_ERR_HIP, "mask kernel failed");
    dm.drop(pat_off); dm.drop(pat);
    return VC_OK;
}

// stage 2: search and pick, a piece of the budget at a time
int dmx_search(DevMem& out, const vc_demux_params* p, Dmx& s, Owned& g) {
    const uint64_t n = s.n, P = s.P;
    const bool all = p->flags & VC_DEMUX_ALL_HITS;
    uint64_t budget = env_mib("VC_DEMUX_BUDGET_MB");
    if (!budget) budget = 256ull << 20;
    // reads of a piece: 2 * reads * P results of 4 bytes within the budget and below 2^31 of them, one read at least
    const uint64_t per_read = 2 * P, reads_per_piece = std::max<uint64_t>(std::min<uint64_t>(budget / 4, (1ull << 31) - 1) / per_read, 1);
    const uint64_t piece = std::min(reads_per_piece, n);
    DevMem dm;
    SearchArgs sa{};
    PickArgs pa{};
    unsigned long long* d_acc = nullptr;
    if (!out.alloc(&s.v_pat, 2 * n) || !out.alloc(&s.v_dist, 2 * n) || !out.alloc(&s.v_start, 2 * n) || !out.alloc(&s.v_end, 2 * n) || !out.alloc(&s.v_second, 2 * n))
        return fail(VC_ERR_HIP, "hipMalloc failed (the views)");
    if (!dm.alloc(&sa.res, piece * per_read) || !dm.alloc(&d_acc, 1) || (all && (!dm.alloc(&sa.all_dist, piece * per_read) || !dm.alloc(&sa.all_end, piece * per_read))))
        return fail(VC_ERR_HIP, "hipMalloc failed (the search table of a piece)");
    if (hipMemset(d_acc, 0, sizeof *d_acc) != hipSuccess) return fail(VC_ERR_HIP, "hipMemset failed");
    if (all) { g.all_dist.resize(n * per_read); g.all_end.resize(n * per_read); }
    sa.P = (uint32_t)P; sa.window = (uint32_t)p->window; sa.off = s.off; sa.bases = s.bases; sa.peq = s.peq; sa.plen = s.plen;
    pa.P = (uint32_t)P; pa.permille = (uint32_t)p->max_err_permille; pa.res = sa.res; pa.off = s.off; pa.bases = s.bases;
    pa.rpeq = s.rpeq; pa.plen = s.plen; pa.label = s.plabel; pa.v_pat = s.v_pat; pa.v_dist = s.v_dist; pa.v_start = s.v_start; pa.v_end = s.v_end;
    pa.v_second = s.v_second; pa.accepted = d_acc;
    for (uint64_t first = 0; first < n; first += piece) {
        const uint64_t cnt = std::min(piece, n - first);
        sa.n_triples = cnt * per_read; sa.view0 = 2 * first;
        pa.n_views = 2 * cnt; pa.view0 = 2 * first;
        hipLaunchKernelGGL(k_dmx_search, dim3(grid(sa.n_triples)), dim3(256), 0, 0, sa);
        hipLaunchKernelGGL(k_dmx_pick, dim3(grid(pa.n_views)), dim3(256), 0, 0, pa);
        if (all && (!to_host(g.all_dist.data() + first * per_read, sa.all_dist, sa.n_triples) || !to_host(g.all_end.data() + first * per_read, sa.all_end, sa.n_triples)))
            return fail(VC_ERR_HIP, "search kernels failed, or copying every hit did");
        ++s.n_budget_pieces;
    }
    if (!ran() || !to_host(&s.accepted, d_acc, 1)) return fail(VC_ERR_HIP, "search kernels failed");
    if (!to_host(g.v_pat, s.v_pat, 2 * n) || !to_host(g.v_dist, s.v_dist, 2 * n) || !to_host(g.v_start, s.v_start, 2 * n) || !to_host(g.v_end, s.v_end, 2 * n) ||
        !to_host(g.v_second, s.v_second, 2 * n))
        return fail(VC_ERR_HIP, "copying the views failed");
    return VC_OK;
}

// stage 3: classes, ranges, piece offsets and groups
int dmx_classify(DevMem& out, const vc_demux_params* p, Dmx& s, Owned& g) {
    const uint64_t n = s.n;
    DevMem dm;
    ClassArgs ca{};
    uint32_t *key2 = nullptr, *val2 = nullptr;
    uint64_t* grp_off = nullptr;
    ca.n = n; ca.min_margin = (uint32_t)p->min_margin; ca.trim = (uint32_t)p->trim; ca.require_both = p->flags & VC_DEMUX_REQUIRE_BOTH;
    ca.off = s.off; ca.plabel = s.plabel; ca.pside = s.pside; ca.v_pat = s.v_pat; ca.v_dist = s.v_dist; ca.v_start = s.v_start; ca.v_end = s.v_end; ca.v_second = s.v_second;
    if (!dm.alloc(&ca.klass, n) || !dm.alloc(&ca.label, n) || !out.alloc(&s.flip, n) || !out.alloc(&s.begin, n) || !dm.alloc(&ca.end, n) || !dm.alloc(&ca.pc_len, n + 1) ||
        !out.alloc(&s.piece_off, n + 1) || !dm.alloc(&ca.key, n) || !dm.alloc(&ca.val, n) || !dm.alloc(&key2, n) || !dm.alloc(&val2, n) || !dm.alloc(&grp_off, (uint64_t)s.n_labels + 1))
        return fail(VC_ERR_HIP, "hipMalloc failed (classes)");
    ca.flip = s.flip; ca.begin = s.begin;
    hipLaunchKernelGGL(k_dmx_classify, dim3(grid(n)), dim3(256), 0, 0, ca);
    if (!exclusive_sum(dm, ca.pc_len, s.piece_off, n + 1)) return fail(VC_ERR_HIP, "scan failed (pieces)");
    if (!sort_pairs(dm, ca.key, key2, ca.val, val2, n, (int)kLabelBits)) return fail(VC_ERR_HIP, "radix sort failed (groups)");
    hipLaunchKernelGGL(k_dmx_first, dim3(grid((uint64_t)s.n_labels + 1)), dim3(256), 0, 0, s.n_labels, n, key2, grp_off);
    if (!ran()) return fail(VC_ERR_HIP, "class kernels failed");
    if (!to_host(g.klass, ca.klass, n) || !to_host(g.label, ca.label, n) || !to_host(g.flip, s.flip, n) || !to_host(g.begin, s.begin, n) || !to_host(g.end, ca.end, n) ||
        !to_host(g.piece_off, s.piece_off, n + 1) || !to_host(g.grp_off, grp_off, (uint64_t)s.n_labels + 1))
        return fail(VC_ERR_HIP, "copying the classes failed");
    if (!to_host(g.grp_reads, val2, g.grp_off[s.n_labels])) return fail(VC_ERR_HIP, "copying the groups failed");
    s.total = g.piece_off[n];
    return VC_OK;
}

// stage 4: the cut (total > 0)
int dmx_cut(const vc_demux_params* p, const vc_demux_in* in, const Dmx& s, Owned& g) {
    DevMem dm;
    CutArgs ca{};
    const uint64_t padded = (s.total + 15) / 16 * 16;
    uint8_t* d_quals = nullptr;
    if (!dm.alloc(&ca.out_bases, padded) || (in->quals && (!dm.alloc(&d_quals, s.n_bytes + 16) || !dm.alloc(&ca.out_quals, padded))))
        return fail(VC_ERR_HIP, "hipMalloc failed (the cut)");
    if (in->quals && !to_device(d_quals, in->quals, s.n_bytes)) return fail(VC_ERR_HIP, "upload failed (the qualities)");
    ca.total = s.total; ca.n = s.n; ca.orient = p->flags & VC_DEMUX_ORIENT; ca.piece_off = s.piece_off; ca.begin = s.begin; ca.flip = s.flip; ca.off = s.off;
    ca.bases = s.bases; ca.quals = d_quals;
    const uint64_t blocks = std::min<uint64_t>((padded / 16 + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(k_dmx_cut, dim3((uint32_t)blocks), dim3(256), 0, 0, ca);
    if (!ran()) return fail(VC_ERR_HIP, "cut kernel failed");
    if (!to_host(g.pc_bases, ca.out_bases, s.total) || (in->quals && !to_host(g.pc_quals, ca.out_quals, s.total))) return fail(VC_ERR_HIP, "copying the cut failed");
    return VC_OK;
}

}  // namespace

extern "C" {

const char* vc_demux_last_error(void) { return g_err.c_str(); }

void vc_demux_release(void) { g_own = Owned{}; }

void vc_demux_default_params(vc_demux_params* p) {
    if (!p) return;
    p->device = 0; p->window = 150; p->max_err_permille = 200; p->min_margin = 2; p->trim = 1; p->flags = 0;
}

int vc_demux(const vc_demux_params* p, const vc_demux_in* in, vc_demux_out* out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!p || !in || !out) return fail(VC_ERR_ARG, "NULL argument");
    if (const char* e = check_args(p, in)) return fail(VC_ERR_ARG, e);
    if (int rc = check_device(p->device, "the demultiplexer", g_err)) return rc;
    if (hipSetDevice(p->device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");

    Owned& g = g_own;
    Dmx s;
    s.n = in->n; s.P = in->n_patterns; s.n_bytes = s.n ? in->off[s.n] : 0;
    for (uint64_t j = 0; j < s.P; ++j) s.n_labels = std::max(s.n_labels, in->label[j] + 1);
    const bool all = p->flags & VC_DEMUX_ALL_HITS;
    g.pc_bases.clear(); g.pc_quals.clear(); g.all_dist.clear(); g.all_end.clear();
    if (s.n == 0) {
        g.v_pat.clear(); g.v_start.clear(); g.v_end.clear(); g.label.clear(); g.begin.clear(); g.end.clear(); g.grp_reads.clear();
        g.v_dist.clear(); g.v_second.clear(); g.klass.clear(); g.flip.clear();
        g.piece_off.assign(1, 0); g.grp_off.assign((size_t)s.n_labels + 1, 0);
    } else {
        DevMem image;                                        // the reads, the patterns and the masks: to the end of the call
        if (int rc = dmx_upload(image, in, s)) return rc;
        DevMem views;
        if (int rc = dmx_search(views, p, s, g)) return rc;
        if (int rc = dmx_classify(views, p, s, g)) return rc;
        if (s.total) if (int rc = dmx_cut(p, in, s, g)) return rc;
    }
    const uint64_t n_triples = 2 * s.n * s.P;
    if (getenv("VC_DEMUX_LOG"))
        fprintf(stderr, "vc_demux: reads=%llu triples=%llu pieces=%llu accepted=%llu\n", (unsigned long long)s.n, (unsigned long long)n_triples,
                (unsigned long long)s.n_budget_pieces, s.accepted);
    // a vector's data() may be NULL when it is empty: every array handed out is a real address
    static const uint32_t none32 = 0;
    static const uint8_t none8 = 0;
    auto p32 = [](const std::vector<uint32_t>& v) { return v.empty() ? &none32 : v.data(); };
    auto p8 = [](const std::vector<uint8_t>& v) { return v.empty() ? &none8 : v.data(); };
    out->v_pat = p32(g.v_pat); out->v_dist = p8(g.v_dist); out->v_start = p32(g.v_start); out->v_end = p32(g.v_end); out->v_second = p8(g.v_second);
    out->klass = p8(g.klass); out->label = p32(g.label); out->flip = p8(g.flip); out->begin = p32(g.begin); out->end = p32(g.end);
    out->piece_off = g.piece_off.data();
    out->pc_bases = in->bases ? p8(g.pc_bases) : nullptr;
    out->pc_quals = in->bases && in->quals ? p8(g.pc_quals) : nullptr;
    out->n_labels = s.n_labels; out->grp_off = g.grp_off.data(); out->grp_reads = p32(g.grp_reads);
    out->all_dist = all ? p8(g.all_dist) : nullptr; out->all_end = all ? p32(g.all_end) : nullptr;
    out->n_reads = s.n; out->n_triples = n_triples; out->n_budget_pieces = s.n_budget_pieces; out->n_accepted = s.accepted;
    return VC_OK;
}

}  // extern "C"
