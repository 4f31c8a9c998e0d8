// Scrubbing of chimeric reads on the device: the step the reference's wrapper leaves to `minimap2 -g | yacrd scrubb`
// (scripts/vechat:187-201).  Intervals "another read overlaps this stretch" go in; the badly covered regions of every read, its
// class and the pieces that are left -- with their bases and qualities cut out -- come back.
//
// yacrd is external to the reference, so, like vc_overlap.hip, the library fixes its OWN rule -- all integer, every case decided,
// written out in include/vechat_hip.h -- and tests/scrub_ref.py restates it position by position without sharing a line with
// this file; tests/test_scrub_gpu.py compares the two array for array.
//
// Test knob, read with getenv on every call:
//   VC_SCRUB_LOG         set: one line per call on stderr, "vc_scrub: intervals=M events=E segments=S regions=R pieces=P"
//
// Kernels (gfx950, wave64); no block waits for another, a thread that needs its neighbour's element reads it from HBM:
//   k_scr_events    interval i -> events 2i (read << 31 | begin, +1) and 2i + 1 (read << 31 | end, -1); hipcub sorts them by key and
//                   one inclusive sum over the deltas is the coverage after every event (every interval opens and closes in one
//                   read, so the sum is 0 at every read boundary: no segmented scan)
//   k_scr_runs      the last event of each run of equal keys is a segment (read, pos, cov) unless pos == len; flag, scan, write
//   k_scr_first     one thread per read: the first segment of the read (lower bound in the sorted segment keys)
//   k_scr_regions   one thread per segment and one per read (the stretch [0, first pos) of a read is an implicit segment of coverage
//                   0): a bad segment OPENS a region when the segment before it in its read is not bad and CLOSES one when the
//                   segment after it is not.  Opens and closes come in the same order, so the r-th close ends the r-th region.
//                   Count pass, one scan of each flag array (opens in the low half of a 64-bit word, closes in the high), write.
//   k_scr_classify  one thread per read over its regions: klass, bad_total, the number of pieces and of their bytes
//   k_scr_pieces    after the scan of those: the pieces and their byte offsets
//   k_scr_cut       the one bandwidth kernel: one thread per 16 output bytes, bases and qualities in one launch
//
// Host: vc_scrub() is the argument checks and four stages -- scr_segments, scr_regions, scr_pieces, scr_cut --, each with its scratch
// in a DevMem of its own.  DevMem, the checked copies and the device check are vc_devutil.h's, the sort and the sums vc_devscan.h's.
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

constexpr uint64_t kPosMask = 0x7FFFFFFFull;          // key = read << 31 | position; a position is at most VC_OVL_MAX_LEN = 2^30

__global__ void k_scr_events(uint64_t m, const uint32_t* rd, const uint32_t* b, const uint32_t* e, ulonglong2* key, int2* delta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t r = (uint64_t)rd[i] << 31;
    key[i] = make_ulonglong2(r | b[i], r | e[i]);
    delta[i] = make_int2(1, -1);
}

// write == 0: flag[i] = 1 where event i is the last of its run of equal keys and its position is inside the read;
// write == 1 (idx = exclusive scan of the flags): the segment of such an event
__global__ void k_scr_runs(uint64_t n_ev, const uint64_t* key, const int32_t* cov, const uint32_t* len, int write, uint32_t* flag,
                           const uint32_t* idx, uint64_t* seg_key, int32_t* seg_cov) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ev) return;
    const uint64_t k = key[i];
    const bool keep = (i + 1 == n_ev || key[i + 1] != k) && (uint32_t)(k & kPosMask) < len[k >> 31];
    if (!write) { flag[i] = keep ? 1u : 0u; return; }
    if (keep) { seg_key[idx[i]] = k; seg_cov[idx[i]] = cov[i]; }
}

// first[r], r = 0 .. n: the first segment whose read is >= r (first[n] = n_seg)
__global__ void k_scr_first(uint64_t n, uint32_t n_seg, const uint64_t* seg_key, uint32_t* first) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const uint64_t want = r << 31;
    uint32_t lo = 0, hi = n_seg;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg_key[mid] < want) lo = mid + 1; else hi = mid;
    }
    first[r] = lo;
}

struct RegionArgs {
    uint64_t n; uint32_t n_seg; int32_t c; int write;
    const uint32_t* len; const uint32_t* first;            // [n], [n + 1]
    const uint64_t* seg_key; const int32_t* seg_cov;       // [n_seg]
    uint64_t* sflag; uint64_t* hflag;                      // [n_seg + 1], [n + 1]: opens | closes << 32, a 0 at the end
    const uint64_t* sscan; const uint64_t* hscan;          // their exclusive scans
    uint32_t* reg_read; uint32_t* reg_begin; uint32_t* reg_end; uint64_t* reg_off;
};

__global__ void k_scr_regions(RegionArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_seg) {                                       // a segment
        const uint32_t j = (uint32_t)i;
        const uint64_t k = a.seg_key[j];
        const uint64_t r = k >> 31;
        const uint32_t pos = (uint32_t)(k & kPosMask), lo = a.first[r], hi = a.first[r + 1];
        const bool bad = a.seg_cov[j] <= a.c;
        const bool prev_bad = j > lo ? a.seg_cov[j - 1] <= a.c : pos > 0;      // in front of the first segment: the implicit one
        const bool next_bad = j + 1 < hi ? a.seg_cov[j + 1] <= a.c : false;
        const bool opens = bad && !prev_bad, closes = bad && !next_bad;
        if (!a.write) { a.sflag[j] = (uint64_t)opens | (uint64_t)closes << 32; return; }
        const uint64_t s = a.sscan[j], h = a.hscan[r + 1];
        if (opens) { const uint32_t at = (uint32_t)s + (uint32_t)h; a.reg_read[at] = (uint32_t)r; a.reg_begin[at] = pos; }
        if (closes) a.reg_end[(uint32_t)(s >> 32) + (uint32_t)(h >> 32)] = j + 1 < hi ? (uint32_t)(a.seg_key[j + 1] & kPosMask) : a.len[r];
        return;
    }
    const uint64_t r = i - a.n_seg;                          // a read: its implicit segment [0, first pos) of coverage 0
    if (r >= a.n) return;
    const uint32_t L = a.len[r], lo = a.first[r], hi = a.first[r + 1];
    const bool has = hi > lo;
    const uint32_t first_pos = has ? (uint32_t)(a.seg_key[lo] & kPosMask) : L;
    const bool opens = L > 0 && first_pos > 0;
    const bool closes = opens && (!has || a.seg_cov[lo] > a.c);
    if (!a.write) {
        a.hflag[r] = (uint64_t)opens | (uint64_t)closes << 32;
        if (r == 0) { a.hflag[a.n] = 0; a.sflag[a.n_seg] = 0; }
        return;
    }
    const uint64_t s = a.sscan[lo], h = a.hscan[r];
    const uint32_t at = (uint32_t)s + (uint32_t)h;
    a.reg_off[r] = at;
    if (r == 0) a.reg_off[a.n] = (uint64_t)(uint32_t)a.sscan[a.n_seg] + (uint32_t)a.hscan[a.n];
    if (opens) { a.reg_read[at] = (uint32_t)r; a.reg_begin[at] = 0; }
    if (closes) a.reg_end[(uint32_t)(s >> 32) + (uint32_t)(h >> 32)] = first_pos;
}

struct PieceArgs {
    uint64_t n; int32_t permille, min_piece; int write;
    const uint32_t* len; const uint64_t* reg_off; const uint32_t* reg_begin; const uint32_t* reg_end;
    uint8_t* klass; uint32_t* bad_total; uint64_t* pcnt; uint64_t* pbytes;       // [n], [n], [n + 1], [n + 1] (a 0 at the end)
    const uint64_t* pidx; const uint64_t* pboff;                                 // exclusive scans of pcnt and pbytes
    uint32_t* pc_read; uint32_t* pc_begin; uint32_t* pc_end; uint64_t* pc_off;
};

// write == 0: k_scr_classify; write == 1: k_scr_pieces.  One thread per read, the same walk over its regions.
__device__ __forceinline__ void scr_read(const PieceArgs& a, uint64_t r) {
    const uint32_t L = a.len[r];
    const uint64_t r0 = a.reg_off[r], r1 = a.reg_off[r + 1];
    int klass;
    if (!a.write) {
        uint64_t total = 0;
        bool inner = false;
        for (uint64_t x = r0; x < r1; ++x) {
            const uint32_t b = a.reg_begin[x], e = a.reg_end[x];
            total += e - b;
            inner = inner || (b > 0 && e < L);
        }
        klass = 1000ull * total > (uint64_t)a.permille * L ? VC_SCRUB_NOT_COVERED : inner ? VC_SCRUB_CHIMERIC : r1 > r0 ? VC_SCRUB_BAD_ENDS : VC_SCRUB_CLEAN;
        a.klass[r] = (uint8_t)klass; a.bad_total[r] = (uint32_t)total;
    } else {
        klass = a.klass[r];
    }
    uint64_t cnt = 0, bytes = 0;
    uint64_t at = a.write ? a.pidx[r] : 0, boff = a.write ? a.pboff[r] : 0;
    if (klass != VC_SCRUB_NOT_COVERED) {
        uint32_t cur = 0;
        for (uint64_t x = r0; x <= r1; ++x) {                // the stretch in front of every region, and the one behind the last
            const uint32_t b = x < r1 ? a.reg_begin[x] : L;
            if (b - cur >= (uint32_t)a.min_piece) {
                if (a.write) { a.pc_read[at] = (uint32_t)r; a.pc_begin[at] = cur; a.pc_end[at] = b; a.pc_off[at] = boff; ++at; boff += b - cur; }
                ++cnt; bytes += b - cur;
            }
            if (x < r1) cur = a.reg_end[x];
        }
    }
    if (!a.write) {
        a.pcnt[r] = cnt; a.pbytes[r] = bytes;
        if (r == 0) { a.pcnt[a.n] = 0; a.pbytes[a.n] = 0; }
    } else if (r == 0) {
        a.pc_off[a.pidx[a.n]] = a.pboff[a.n];
    }
}
__global__ void k_scr_classify(PieceArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < a.n) scr_read(a, r);
}
__global__ void k_scr_pieces(PieceArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < a.n) scr_read(a, r);
}

struct CutArgs {
    uint64_t total; uint64_t n_pieces;                     // bytes of all pieces; pieces (>= 1)
    const uint64_t* pc_off; const uint32_t* pc_read; const uint32_t* pc_begin;
    const uint64_t* off;                                   // [n + 1] the reads in the image
    const uint8_t* bases; const uint8_t* quals;            // the image (16 bytes of padding behind it); quals may be NULL
    uint8_t* out_bases; uint8_t* out_quals;
};

// 16 bytes from any address: one 16-byte load where the address allows it, else the five aligned words around them, shifted
__device__ __forceinline__ uint4 scr_load16(const uint8_t* base, uint64_t s) {
    if ((s & 15) == 0) return *reinterpret_cast<const uint4*>(base + s);
    const uint32_t sh = (uint32_t)(s & 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (s - sh));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];      // w4: at most 3 bytes past the 16, inside the padding at worst
    return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh),
                      __builtin_amdgcn_alignbyte(w4, w3, sh));
}

__global__ __launch_bounds__(256) void k_scr_cut(CutArgs a) {
    const uint64_t n_chunks = (a.total + 15) / 16;
    for (uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < n_chunks; ch += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = ch * 16, o1 = min(o0 + 16, a.total);
        uint64_t lo = 0, hi = a.n_pieces;                    // the piece of byte o0: the last one that starts at or before it
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.pc_off[mid] <= o0) lo = mid; else hi = mid;
        }
        uint64_t p = lo;
        if (a.pc_off[p + 1] >= o0 + 16) {                    // the whole chunk lies in one piece: one aligned 16-byte store
            const uint64_t s = a.off[a.pc_read[p]] + a.pc_begin[p] + (o0 - a.pc_off[p]);
            reinterpret_cast<uint4*>(a.out_bases)[ch] = scr_load16(a.bases, s);
            if (a.quals) reinterpret_cast<uint4*>(a.out_quals)[ch] = scr_load16(a.quals, s);
            continue;
        }
        for (uint64_t o = o0; o < o1; ++o) {                 // the tail of a piece and the heads of the next: byte by byte
            while (o >= a.pc_off[p + 1]) ++p;
            const uint64_t s = a.off[a.pc_read[p]] + a.pc_begin[p] + (o - a.pc_off[p]);
            a.out_bases[o] = a.bases[s];
            if (a.quals) a.out_quals[o] = a.quals[s];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// what the library owns between calls (one set per process, like the vc_overlap_out arrays)
struct Owned {
    std::vector<uint32_t> reg_read, reg_begin, reg_end, bad_total, pc_read, pc_begin, pc_end;
    std::vector<uint64_t> reg_off, pc_off;
    std::vector<uint8_t> klass, pc_bases, pc_quals;
};
Owned g_own;

const char* check_args(const vc_scrub_params* p, const vc_scrub_in* in) {
    if (!in->len && in->n) return "NULL argument: reads without lengths";
    if (in->m && (!in->read || !in->begin || !in->end)) return "NULL argument: intervals without an array";
    if (in->bases && !in->off) return "NULL argument: bases without offsets";
    if (in->quals && !in->bases) return "NULL argument: qualities without bases";
    if (in->off) {
        if (in->off[0] != 0) return "offsets do not start at 0";
        for (uint64_t r = 0; r < in->n; ++r) if (in->off[r + 1] < in->off[r]) return "offsets decrease";
        for (uint64_t r = 0; r < in->n; ++r) if (in->off[r + 1] - in->off[r] != in->len[r]) return "offsets disagree with the lengths";
    }
    if (p->coverage < 0 || p->coverage > (1 << 30)) return "coverage outside 0..2^30";
    if (p->max_bad_permille < 0 || p->max_bad_permille > 1000) return "max_bad_permille outside 0..1000";
    if (p->min_piece < 1) return "min_piece below 1";
    for (uint64_t i = 0; i < in->m; ++i) {
        if (in->read[i] >= in->n) return "an interval of a read that is not there";
        if (in->begin[i] >= in->end[i]) return "an interval that is empty";
        if (in->end[i] > in->len[in->read[i]]) return "an interval outside its read";
    }
    if (in->n > VC_OVL_MAX_SEQS) return "more reads than the envelope (VC_OVL_MAX_SEQS)";
    for (uint64_t r = 0; r < in->n; ++r) if (in->len[r] > VC_OVL_MAX_LEN) return "a read longer than the envelope (VC_OVL_MAX_LEN)";
    if (in->m >= (1ull << 30)) return "more intervals than the envelope (2 m < 2^31)";
    return nullptr;
}

// The device arrays that cross the stages below, and their counts.  Every stage takes the DevMem that its results go into and
// keeps its scratch in one of its own, so the scratch is gone when the stage returns; it returns VC_OK or the code of fail().
struct Scr {
    uint64_t n = 0, m = 0, n_ev = 0;
    int32_t coverage = 0, permille = 0, min_piece = 0;
    uint32_t* len = nullptr;                                                      // [n], the whole call
    uint64_t n_seg = 0; uint64_t* seg_key = nullptr; int32_t* seg_cov = nullptr;  // segments -> regions
    uint64_t n_reg = 0; uint32_t *reg_read = nullptr, *reg_begin = nullptr, *reg_end = nullptr; uint64_t* reg_off = nullptr;   // -> pieces
    uint64_t n_pc = 0, total = 0; uint32_t *pc_read = nullptr, *pc_begin = nullptr; uint64_t* pc_off = nullptr;               // -> cut
};

// stage 1: intervals -> sorted events -> the coverage after each -> segments
int scr_segments(DevMem& out, const vc_scrub_in* in, Scr& s) {
    const uint64_t n = s.n, m = s.m, n_ev = s.n_ev;
    if (m == 0) return out.alloc(&s.seg_key, 1) && out.alloc(&s.seg_cov, 1) ? VC_OK : fail(VC_ERR_HIP, "hipMalloc failed (segments)");
    DevMem dm;
    uint32_t *d_rd = nullptr, *d_b = nullptr, *d_e = nullptr, *flag = nullptr, *idx = nullptr;
    uint64_t *key = nullptr, *key2 = nullptr;
    int32_t *delta = nullptr, *delta2 = nullptr;
    if (!dm.alloc(&d_rd, m, in->read) || !dm.alloc(&d_b, m, in->begin) || !dm.alloc(&d_e, m, in->end)) return fail(VC_ERR_HIP, "hipMalloc or upload failed (intervals)");
    if (!dm.alloc(&key, n_ev) || !dm.alloc(&key2, n_ev) || !dm.alloc(&delta, n_ev) || !dm.alloc(&delta2, n_ev)) return fail(VC_ERR_HIP, "hipMalloc failed (events)");
    hipLaunchKernelGGL(k_scr_events, dim3(grid(m)), dim3(256), 0, 0, m, d_rd, d_b, d_e, (ulonglong2*)key, (int2*)delta);
    int bits = 32;
    while (bits < 62 && ((n - 1) >> (bits - 31)) != 0) ++bits;
    if (!sort_pairs(dm, key, key2, delta, delta2, n_ev, bits)) return fail(VC_ERR_HIP, "radix sort failed (events)");
    dm.drop(key); dm.drop(d_rd); dm.drop(d_b); dm.drop(d_e);                      // the peak of the call is the sort: nothing of it stays for the runs
    int32_t* cov = delta;                                                         // the unsorted deltas are done with
    if (!inclusive_sum(dm, delta2, cov, n_ev)) return fail(VC_ERR_HIP, "scan failed (coverage)");
    dm.drop(delta2);
    // the runs of equal keys -> segments
    if (!dm.alloc(&flag, n_ev + 1) || !dm.alloc(&idx, n_ev + 1)) return fail(VC_ERR_HIP, "hipMalloc failed (runs)");
    (void)hipMemset(flag + n_ev, 0, 4);
    hipLaunchKernelGGL(k_scr_runs, dim3(grid(n_ev)), dim3(256), 0, 0, n_ev, key2, cov, s.len, 0, flag, idx, s.seg_key, s.seg_cov);
    if (!exclusive_sum(dm, flag, idx, n_ev + 1)) return fail(VC_ERR_HIP, "scan failed (runs)");
    uint32_t s32 = 0;
    if (!to_host(&s32, idx + n_ev, 1)) return fail(VC_ERR_HIP, "event kernels failed");
    s.n_seg = s32;
    if (!out.alloc(&s.seg_key, s.n_seg) || !out.alloc(&s.seg_cov, s.n_seg)) return fail(VC_ERR_HIP, "hipMalloc failed (segments)");
    hipLaunchKernelGGL(k_scr_runs, dim3(grid(n_ev)), dim3(256), 0, 0, n_ev, key2, cov, s.len, 1, flag, idx, s.seg_key, s.seg_cov);
    return ran() ? VC_OK : fail(VC_ERR_HIP, "event kernels failed");
}

// stage 2: segments -> regions
int scr_regions(DevMem& out, Scr& s) {
    const uint64_t n = s.n, n_seg = s.n_seg;
    DevMem dm;
    RegionArgs ra{};
    uint32_t* first = nullptr;
    uint64_t *sflag = nullptr, *hflag = nullptr, *sscan = nullptr, *hscan = nullptr;
    if (!dm.alloc(&first, n + 1) || !dm.alloc(&sflag, n_seg + 1) || !dm.alloc(&hflag, n + 1) || !dm.alloc(&sscan, n_seg + 1) || !dm.alloc(&hscan, n + 1) || !out.alloc(&s.reg_off, n + 1))
        return fail(VC_ERR_HIP, "hipMalloc failed (regions)");
    hipLaunchKernelGGL(k_scr_first, dim3(grid(n + 1)), dim3(256), 0, 0, n, (uint32_t)n_seg, s.seg_key, first);
    ra.n = n; ra.n_seg = (uint32_t)n_seg; ra.c = s.coverage; ra.write = 0; ra.len = s.len; ra.first = first; ra.seg_key = s.seg_key; ra.seg_cov = s.seg_cov;
    ra.sflag = sflag; ra.hflag = hflag; ra.sscan = sscan; ra.hscan = hscan; ra.reg_off = s.reg_off;
    hipLaunchKernelGGL(k_scr_regions, dim3(grid(n_seg + n)), dim3(256), 0, 0, ra);
    if (!exclusive_sum(dm, sflag, sscan, n_seg + 1) || !exclusive_sum(dm, hflag, hscan, n + 1)) return fail(VC_ERR_HIP, "scan failed (regions)");
    uint64_t s_last = 0, h_last = 0;
    if (!to_host(&s_last, sscan + n_seg, 1) || !to_host(&h_last, hscan + n, 1)) return fail(VC_ERR_HIP, "region kernels failed");
    s.n_reg = (uint64_t)(uint32_t)s_last + (uint32_t)h_last;
    if (s.n_reg != (s_last >> 32) + (h_last >> 32)) return fail(VC_ERR_HIP, "region kernels failed: opens and closes differ");
    if (!out.alloc(&s.reg_read, s.n_reg) || !out.alloc(&s.reg_begin, s.n_reg) || !out.alloc(&s.reg_end, s.n_reg)) return fail(VC_ERR_HIP, "hipMalloc failed (regions)");
    ra.reg_read = s.reg_read; ra.reg_begin = s.reg_begin; ra.reg_end = s.reg_end; ra.write = 1;
    hipLaunchKernelGGL(k_scr_regions, dim3(grid(n_seg + n)), dim3(256), 0, 0, ra);
    return ran() ? VC_OK : fail(VC_ERR_HIP, "region kernels failed");          // the flags and scans go now: the launch must be through with them
}

// stage 3: regions -> classes and pieces, and every table of the call on the host
int scr_pieces(DevMem& out, Scr& s, Owned& g) {
    const uint64_t n = s.n;
    DevMem dm;
    PieceArgs pa{};
    uint64_t *pidx = nullptr, *pboff = nullptr;
    pa.n = n; pa.permille = s.permille; pa.min_piece = s.min_piece; pa.write = 0; pa.len = s.len;
    pa.reg_off = s.reg_off; pa.reg_begin = s.reg_begin; pa.reg_end = s.reg_end;
    if (!dm.alloc(&pa.klass, n) || !dm.alloc(&pa.bad_total, n) || !dm.alloc(&pa.pcnt, n + 1) || !dm.alloc(&pa.pbytes, n + 1) || !dm.alloc(&pidx, n + 1) || !dm.alloc(&pboff, n + 1))
        return fail(VC_ERR_HIP, "hipMalloc failed (classes)");
    hipLaunchKernelGGL(k_scr_classify, dim3(grid(n)), dim3(256), 0, 0, pa);
    if (!exclusive_sum(dm, pa.pcnt, pidx, n + 1) || !exclusive_sum(dm, pa.pbytes, pboff, n + 1)) return fail(VC_ERR_HIP, "scan failed (pieces)");
    if (!to_host(&s.n_pc, pidx + n, 1) || !to_host(&s.total, pboff + n, 1)) return fail(VC_ERR_HIP, "region or class kernels failed");
    pa.pidx = pidx; pa.pboff = pboff; pa.write = 1;
    if (!out.alloc(&s.pc_read, s.n_pc) || !out.alloc(&s.pc_begin, s.n_pc) || !dm.alloc(&pa.pc_end, s.n_pc) || !out.alloc(&s.pc_off, s.n_pc + 1)) return fail(VC_ERR_HIP, "hipMalloc failed (pieces)");
    pa.pc_read = s.pc_read; pa.pc_begin = s.pc_begin; pa.pc_off = s.pc_off;
    hipLaunchKernelGGL(k_scr_pieces, dim3(grid(n)), dim3(256), 0, 0, pa);
    if (!ran()) return fail(VC_ERR_HIP, "piece kernels failed");
    if (!to_host(g.reg_read, s.reg_read, s.n_reg) || !to_host(g.reg_begin, s.reg_begin, s.n_reg) || !to_host(g.reg_end, s.reg_end, s.n_reg) ||
        !to_host(g.reg_off, s.reg_off, n + 1) || !to_host(g.klass, pa.klass, n) || !to_host(g.bad_total, pa.bad_total, n) ||
        !to_host(g.pc_read, s.pc_read, s.n_pc) || !to_host(g.pc_begin, s.pc_begin, s.n_pc) || !to_host(g.pc_end, pa.pc_end, s.n_pc) ||
        !to_host(g.pc_off, s.pc_off, s.n_pc + 1))
        return fail(VC_ERR_HIP, "copying the regions and pieces failed");
    return VC_OK;
}

// stage 4: the cut (total > 0, so there is a piece)
int scr_cut(const vc_scrub_in* in, const Scr& s, Owned& g) {
    DevMem dm;
    CutArgs ca{};
    const uint64_t n_bytes = in->off[s.n], padded = (s.total + 15) / 16 * 16;
    uint8_t *d_bases = nullptr, *d_quals = nullptr;
    uint64_t* d_off = nullptr;
    if (!dm.alloc(&d_off, s.n + 1, in->off) || !dm.alloc(&d_bases, n_bytes + 16) || !dm.alloc(&ca.out_bases, padded) ||
        (in->quals && (!dm.alloc(&d_quals, n_bytes + 16) || !dm.alloc(&ca.out_quals, padded))))
        return fail(VC_ERR_HIP, "hipMalloc failed (the read image and the cut)");
    if (!to_device(d_bases, in->bases, n_bytes) || (in->quals && !to_device(d_quals, in->quals, n_bytes))) return fail(VC_ERR_HIP, "upload failed (the read image)");
    ca.total = s.total; ca.n_pieces = s.n_pc; ca.pc_off = s.pc_off; ca.pc_read = s.pc_read; ca.pc_begin = s.pc_begin; ca.off = d_off;
    ca.bases = d_bases; ca.quals = d_quals;
    const uint64_t blocks = std::min<uint64_t>((padded / 16 + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(k_scr_cut, dim3((uint32_t)blocks), dim3(256), 0, 0, ca);
    if (!ran()) return fail(VC_ERR_HIP, "cut kernel failed");
    if (!to_host(g.pc_bases, ca.out_bases, s.total) || (in->quals && !to_host(g.pc_quals, ca.out_quals, s.total))) return fail(VC_ERR_HIP, "copying the cut failed");
    return VC_OK;
}

}  // namespace

extern "C" {

const char* vc_scrub_last_error(void) { return g_err.c_str(); }

void vc_scrub_release(void) { g_own = Owned{}; }

void vc_scrub_default_params(vc_scrub_params* p) {
    if (!p) return;
    p->device = 0; p->coverage = 0; p->max_bad_permille = 400; p->min_piece = 1;
}

int vc_scrub(const vc_scrub_params* p, const vc_scrub_in* in, vc_scrub_out* out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!p || !in || !out) return fail(VC_ERR_ARG, "NULL argument");
    if (const char* e = check_args(p, in)) return fail(VC_ERR_ARG, e);
    if (int rc = check_device(p->device, "the scrubber", g_err)) return rc;
    if (hipSetDevice(p->device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");

    Owned& g = g_own;
    Scr s;
    s.n = in->n; s.m = in->m; s.n_ev = 2 * in->m; s.coverage = p->coverage; s.permille = p->max_bad_permille; s.min_piece = p->min_piece;
    const bool cut = in->bases != nullptr;
    g.pc_bases.clear(); g.pc_quals.clear();
    if (s.n == 0) {
        g.reg_read.clear(); g.reg_begin.clear(); g.reg_end.clear(); g.bad_total.clear(); g.pc_read.clear(); g.pc_begin.clear(); g.pc_end.clear();
        g.klass.clear();
        g.reg_off.assign(1, 0); g.pc_off.assign(1, 0);
    } else {
        DevMem pieces;                                       // the lengths and the pieces: to the end of the call
        if (!pieces.alloc(&s.len, s.n, in->len)) return fail(VC_ERR_HIP, "hipMalloc or upload failed (lengths)");
        {
            DevMem regions;                                  // gone before the cut uploads the read image
            {
                DevMem segments;                             // gone before the pieces are built
                if (int rc = scr_segments(segments, in, s)) return rc;
                if (int rc = scr_regions(regions, s)) return rc;
            }
            if (int rc = scr_pieces(pieces, s, g)) return rc;
        }
        if (cut && s.total) if (int rc = scr_cut(in, s, g)) return rc;
    }
    if (getenv("VC_SCRUB_LOG"))
        fprintf(stderr, "vc_scrub: intervals=%llu events=%llu segments=%llu regions=%llu pieces=%llu\n", (unsigned long long)s.m, (unsigned long long)s.n_ev,
                (unsigned long long)s.n_seg, (unsigned long long)s.n_reg, (unsigned long long)s.n_pc);
    // a vector's data() may be NULL when it is empty: every array handed out is a real address
    static const uint32_t none32 = 0;
    static const uint8_t none8 = 0;
    auto p32 = [](const std::vector<uint32_t>& v) { return v.empty() ? &none32 : v.data(); };
    auto p8 = [](const std::vector<uint8_t>& v) { return v.empty() ? &none8 : v.data(); };
    out->n_regions = s.n_reg; out->reg_read = p32(g.reg_read); out->reg_begin = p32(g.reg_begin); out->reg_end = p32(g.reg_end); out->reg_off = g.reg_off.data();
    out->klass = p8(g.klass); out->bad_total = p32(g.bad_total);
    out->n_pieces = s.n_pc; out->pc_read = p32(g.pc_read); out->pc_begin = p32(g.pc_begin); out->pc_end = p32(g.pc_end); out->pc_off = g.pc_off.data();
    out->pc_bases = cut ? p8(g.pc_bases) : nullptr;
    out->pc_quals = cut && in->quals ? p8(g.pc_quals) : nullptr;
    out->n_intervals = s.m; out->n_events = s.n_ev; out->n_segments = s.n_seg;
    return VC_OK;
}

}  // extern "C"
