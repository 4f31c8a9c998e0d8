// All-vs-all read overlaps on the device: the stage the reference leaves to `minimap2 -x ava-* | awk | fpa`.
//
// There is nothing to pin this stage to: the overlapper is an external command for the reference too.  So, as vc_align.hip
// does for the alignment path, the library fixes its OWN rule -- all integer, every tie decided, written out in
// include/vechat_hip.h -- and tests/overlap_ref.py restates it on the CPU without sharing a line with this file;
// tests/test_overlap_gpu.py compares the two array for array.
//
// Test knobs, read with getenv on every vc_overlap call; unset, each leaves the behaviour as it is:
//   VC_OVL_BUDGET_MB=x   the anchor budget of one target piece in MiB, instead of half of the free device memory
//   VC_OVL_LOG           set: one line per piece on stderr, "vc_overlap: piece first=T targets=N anchors=A keys=K records=R"
//
// Kernels (gfx950, wave64):
//   k_ovl_sketch   one block per stretch of 256 positions of one sequence.  The 2-bit codes of the stretch and its halo
//                  (k + w - 2 bases to the left, w - 1 to the right) and the hashes of their k-mers sit in LDS; one thread per
//                  position decides "leftmost minimum of some window"; ballot + prefix within the block.  Run twice: count,
//                  then (after a scan of the block counts) write, so the table comes out sorted by (sequence, position).
//   k_ovl_heads / k_ovl_bounds   flag-and-scan: the bounds of the runs of equal keys in a sorted array (hash buckets, chain keys)
//   k_ovl_count    one thread per target entry: the anchors it makes with the query entries of its bucket
//   k_ovl_emit     the same walk, writing the anchors at the offsets the scan of the counts gave
//   k_ovl_chain    one wave per key (t_id, q_id, strand).  The anchors are walked in order; lane l evaluates predecessor
//                  i - 1 - l; f and the positions of the last 64 anchors live in registers (anchor i in lane i & 63, fetched
//                  with a lane shuffle); a wave maximum and a ballot apply the tie rule.  f and pred of every anchor go to HBM
//                  for the walk back, which lane 0 does together with the record.
//   Sorting and scanning are hipcub's (DeviceRadixSort, DeviceScan); both are stable / deterministic for integers.
//
// Host: the device buffers of a scope (DevMem), the checked copies and the device check are vc_devutil.h's; the sort and the
// prefix sums are vc_devscan.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vechat_hip.h"

#include "vc_devscan.h"

namespace {

constexpr int kStretch = 256;                         // positions per sketch block (= its threads)
constexpr int kMaxK = 28, kMaxW = 64;
constexpr int kCodes = kStretch + kMaxK + 2 * kMaxW - 3;   // codes of a stretch and its halo
constexpr int kHashes = kStretch + 2 * (kMaxW - 1);
constexpr uint64_t kInf = 1ull << 62;                 // a k-mer equal to its reverse complement: holds its place, never the minimum
constexpr uint64_t kNone = ~0ull;                     // no k-mer ends here: no window reaches across

__host__ __device__ inline uint64_t ovl_mix(uint64_t key, uint64_t mask) {       // Wang's invertible mix on 2k bits (the header writes it out)
    key = (~key + (key << 21)) & mask;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & mask;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & mask;
    key = key ^ key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

struct SketchArgs {
    uint32_t n_blocks; int k, w; int write;
    const uint32_t* blk_seq; const uint32_t* blk_start;     // [n_blocks]
    const uint64_t* off; const uint8_t* bases;              // the sequences, back to back
    uint64_t* blk_cnt;                                      // [n_blocks] out when !write
    const uint64_t* blk_off;                                // [n_blocks] in when write
    uint64_t* hash; uint32_t* seq; uint32_t* pos; uint8_t* strand;
};

__global__ __launch_bounds__(kStretch) void k_ovl_sketch(SketchArgs a) {
    __shared__ uint8_t codes[kCodes];
    __shared__ uint64_t hsh[kHashes];
    __shared__ uint8_t hstr[kHashes];
    __shared__ uint32_t wcnt[kStretch / 64];
    const uint32_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int tid = threadIdx.x, k = a.k, w = a.w;
    const uint32_t sq = a.blk_seq[b];
    const int64_t start = a.blk_start[b];
    const uint64_t o = a.off[sq];
    const int64_t len = (int64_t)(a.off[sq + 1] - o);
    const int nh = kStretch + 2 * (w - 1), nc = nh + k - 1;
    const int64_t h0 = start - (w - 1), c0 = h0 - (k - 1);   // the positions of hsh[0] and codes[0]
    for (int ci = tid; ci < nc; ci += kStretch) {
        const int64_t p = c0 + ci;
        uint8_t c = 4;
        if (p >= 0 && p < len) {
            const uint8_t ch = a.bases[o + (uint64_t)p] & 0xDF;           // upper case
            c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
        }
        codes[ci] = c;
    }
    __syncthreads();
    const uint64_t mask = (1ull << (2 * k)) - 1;
    for (int hi = tid; hi < nh; hi += kStretch) {            // the k-mer whose last base is position h0 + hi: codes[hi .. hi + k - 1]
        uint64_t fw = 0, rv = 0;
        bool ok = true;
        for (int x = 0; x < k; ++x) {
            const uint32_t c = codes[hi + x];
            ok = ok && c < 4;
            fw = (fw << 2) | (c & 3);
            rv = (rv >> 2) | ((uint64_t)(3 - (c & 3)) << (2 * (k - 1)));
        }
        uint64_t h = kNone;
        uint8_t st = 0;
        if (ok) {
            if (fw == rv) h = kInf;
            else { st = fw < rv ? 0 : 1; h = ovl_mix(fw < rv ? fw : rv, mask); }
        }
        hsh[hi] = h; hstr[hi] = st;
    }
    __syncthreads();
    const int64_t p = start + tid;
    const int hi = tid + w - 1;
    bool is_min = false;
    uint64_t h = kNone;
    if (p < len) {
        h = hsh[hi];
        if (h < kInf) {
            // leftmost minimum of the window [s, s + w - 1] for some s: strictly smaller than what lies left of it in the window, not
            // larger than what lies right; L and R count how far that holds (never across a position without a k-mer)
            int L = 0, R = 0;
            while (L < w - 1 && hsh[hi - 1 - L] != kNone && hsh[hi - 1 - L] > h) ++L;
            while (R < w - 1 && hsh[hi + 1 + R] != kNone && hsh[hi + 1 + R] >= h) ++R;
            is_min = L + R >= w - 1;
        }
    }
    const unsigned long long bal = __ballot(is_min);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wcnt[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int x = 0; x < kStretch / 64; ++x) { before += x < wv ? wcnt[x] : 0; total += wcnt[x]; }
    if (!a.write) {
        if (tid == 0) a.blk_cnt[b] = total;
        return;
    }
    if (is_min) {
        const uint64_t at = a.blk_off[b] + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
        a.hash[at] = h; a.seq[at] = sq; a.pos[at] = (uint32_t)p; a.strand[at] = hstr[hi];
    }
}

__global__ void k_ovl_iota(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// flag-and-scan, step 1: 1 where a run of equal keys starts
__global__ void k_ovl_heads(const uint64_t* key, uint32_t n, uint32_t* flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// step 3 (after the inclusive scan of the flags, id = 1-based run number): start[r] = first element of run r, start[runs] = n
__global__ void k_ovl_bounds(const uint64_t* key, const uint32_t* id, uint32_t n, uint32_t* start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || key[i] != key[i - 1]) start[id[i] - 1] = i;
    if (i == n - 1) start[id[i]] = n;
}

__global__ void k_ovl_gather(const uint64_t* src, uint64_t n_src, uint64_t last, const uint64_t* idx, uint32_t n, uint64_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = idx[i] < n_src ? src[idx[i]] : last;
}

struct SeedArgs {
    uint32_t n;                       // entries of the table (targets first, then the queries unless same_set)
    uint32_t n_t;                     // entries that play the target role (= n with same_set)
    int same_set, max_occ, k;
    const uint32_t* perm;             // [n] sorted by hash (stable): position -> entry
    const uint32_t* bid;              // [n] 1-based bucket of a sorted position
    const uint32_t* bstart;           // [buckets + 1]
    const uint32_t* seq; const uint32_t* pos; const uint8_t* strand;     // the table, by entry
    const uint64_t* off;              // sequence offsets (lengths), by table sequence id
    uint32_t n_targets;               // sequences of the target set: a query's id is its table id minus this, unless same_set
    uint64_t* cnt;                    // [n_t] anchors of a target entry
    uint32_t* lo; uint32_t* hi;       // [n_t] its bucket, as sorted positions
    // emit
    uint32_t e0, e1;                  // the piece's target entries
    const uint64_t* cum;              // [n_t] exclusive scan of cnt
    uint64_t* khi; uint64_t* klo;     // anchors: (t_id << 32 | q_id << 1 | strand), (t_pos << 32 | q_pos)
};

__global__ void k_ovl_count(SeedArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t e = a.perm[i];
    if (e >= a.n_t) return;
    const uint32_t bs = a.bstart[a.bid[i] - 1], be = a.bstart[a.bid[i]];
    uint64_t c = 0;
    if (be - bs <= (uint32_t)a.max_occ) {
        const uint32_t mine = a.seq[e];
        for (uint32_t j = bs; j < be; ++j) {
            const uint32_t f = a.perm[j];
            c += a.same_set ? (a.seq[f] != mine) : (f >= a.n_t);
        }
    }
    a.cnt[e] = c; a.lo[e] = bs; a.hi[e] = be;
}

__global__ void k_ovl_emit(SeedArgs a) {
    const uint32_t e = a.e0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.e1 || a.cnt[e] == 0) return;
    uint64_t at = a.cum[e] - a.cum[a.e0];
    const uint32_t t_id = a.seq[e], t_pos = a.pos[e], t_st = a.strand[e];
    for (uint32_t j = a.lo[e]; j < a.hi[e]; ++j) {
        const uint32_t f = a.perm[j];
        const uint32_t fs = a.seq[f];
        if (a.same_set ? (fs == t_id) : (f < a.n_t)) continue;
        const uint32_t rel = t_st ^ a.strand[f];
        uint32_t q_pos = a.pos[f];
        if (rel) q_pos = (uint32_t)(a.off[fs + 1] - a.off[fs]) - q_pos + (uint32_t)a.k - 2;   // the k-mer's last base on the reversed query
        const uint32_t q_id = a.same_set ? fs : fs - a.n_targets;
        a.khi[at] = ((uint64_t)t_id << 32) | ((uint64_t)q_id << 1) | rel;
        a.klo[at] = ((uint64_t)t_pos << 32) | q_pos;
        ++at;
    }
}

struct OvlRec { int32_t q_id, t_id, strand, q_begin, q_end, t_begin, t_end, n_anchors, score, matches, block; };

struct ChainArgs {
    uint32_t n_keys;
    const uint32_t* kstart;           // [n_keys + 1]
    const uint64_t* khi; const uint64_t* klo;
    int32_t* f; int32_t* pred;        // [anchors]
    int k, max_gap, bandwidth, min_chain_score, min_anchors, min_overlap, drop_internal, same_set;
    const uint64_t* off; uint32_t n_targets;
    OvlRec* rec; uint32_t* n_rec;     // [n_keys] at most, appended
};

__device__ __forceinline__ int ovl_step(int ti, int qi, int tj, int qj, int fj, const ChainArgs& a, int* gain_out) {
    const int dt = ti - tj, dq = qi - qj;
    if (dt <= 0 || dq <= 0 || dt > a.max_gap || dq > a.max_gap) return INT_MIN;
    const int d = dt > dq ? dt - dq : dq - dt;
    if (d > a.bandwidth) return INT_MIN;
    const int gain = min(min(dt, dq), a.k);
    const int cost = d ? (d * a.k) / 100 + (31 - __clz(d)) / 2 : 0;
    if (gain_out) *gain_out = gain;
    return fj + gain - cost;
}

__global__ __launch_bounds__(64) void k_ovl_chain(ChainArgs a) {
    const uint32_t key = blockIdx.x;
    if (key >= a.n_keys) return;
    const int lane = threadIdx.x & 63;
    const uint32_t s = a.kstart[key], n = a.kstart[key + 1] - s;
    if (n < (uint32_t)a.min_anchors) return;                 // a chain has no more anchors than its key
    int rf = 0, rt = 0, rq = 0;                              // anchor i of the last 64 lives in lane i & 63
    int best = -1;
    uint32_t best_i = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t cnt = min(64u, n - base);
        const uint64_t kl = (uint32_t)lane < cnt ? a.klo[s + base + lane] : 0ull;
        const int tn = (int)(kl >> 32), qn = (int)(uint32_t)kl;
        for (uint32_t r = 0; r < cnt; ++r) {
            const uint32_t i = base + r;
            const int ti = __shfl(tn, (int)r), qi = __shfl(qn, (int)r);
            const int64_t j = (int64_t)i - 1 - lane;
            const int src = (int)(j & 63);
            const int fj = __shfl(rf, src), tj = __shfl(rt, src), qj = __shfl(rq, src);
            int cand = INT_MIN;
            if (j >= 0) cand = ovl_step(ti, qi, tj, qj, fj, a, nullptr);
            int m = cand;
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) m = max(m, __shfl_xor(m, x));
            const unsigned long long who = __ballot(cand == m);      // the largest j is the lowest lane
            int f = a.k, p = -1;
            if (m > a.k) { f = m; p = (int)i - 1 - (__ffsll((long long)who) - 1); }
            if ((uint32_t)lane == r) { rf = f; rt = ti; rq = qi; }
            if (lane == 0) { a.f[s + i] = f; a.pred[s + i] = p; }
            if (f > best) { best = f; best_i = i; }
        }
    }
    if (lane != 0) return;
    // the walk back from the best end (ties: the smallest i), and the record
    uint32_t i = best_i;
    int n_a = 0, matches = a.k;
    const uint64_t last = a.klo[s + i];
    uint64_t cur = last;
    for (;;) {
        ++n_a;
        const int p = a.pred[s + i];
        if (p < 0) break;
        const uint64_t pv = a.klo[s + (uint32_t)p];
        int gain = 0;
        (void)ovl_step((int)(cur >> 32), (int)(uint32_t)cur, (int)(pv >> 32), (int)(uint32_t)pv, 0, a, &gain);
        matches += gain;
        cur = pv; i = (uint32_t)p;
    }
    if (best < a.min_chain_score || n_a < a.min_anchors) return;
    const uint64_t kh = a.khi[s];
    const uint32_t t_id = (uint32_t)(kh >> 32), q_id = (uint32_t)(kh >> 1) & 0x7FFFFFFFu, strand = (uint32_t)kh & 1u;
    const uint32_t q_seq = a.same_set ? q_id : q_id + a.n_targets;
    const int t_len = (int)(a.off[t_id + 1] - a.off[t_id]), q_len = (int)(a.off[q_seq + 1] - a.off[q_seq]);
    int t_begin = (int)(cur >> 32) - a.k + 1, t_end = (int)(last >> 32) + 1;
    int qb = (int)(uint32_t)cur - a.k + 1, qe = (int)(uint32_t)last + 1;             // in the query's orientation
    int block = max(qe - qb, t_end - t_begin);
    if (block < a.min_overlap) return;
    if (a.drop_internal) {
        const int left = min(qb, t_begin), right = min(q_len - qe, t_len - t_end);
        // the alignment reaches beyond the outermost shared minimizer: each end is granted three mean anchor spacings of the chain
        const int slack = (int)(3ll * block / n_a);
        const int l2 = max(left - slack, 0), r2 = max(right - slack, 0);
        const long long aligned = (long long)block + (left - l2) + (right - r2);
        if (l2 > 1000 || r2 > 1000 || aligned * 5 < (aligned + l2 + r2) * 4) return;
        // what is left is a dovetail or a containment up to its overhangs: the ends move out along the end diagonals to the nearer read end
        qb -= left; t_begin -= left; qe += right; t_end += right;
        block = max(qe - qb, t_end - t_begin);
    }
    OvlRec rec;
    rec.q_id = (int32_t)q_id; rec.t_id = (int32_t)t_id; rec.strand = (int32_t)strand;
    rec.q_begin = strand ? q_len - qe : qb; rec.q_end = strand ? q_len - qb : qe;
    rec.t_begin = t_begin; rec.t_end = t_end; rec.n_anchors = n_a; rec.score = best; rec.matches = matches; rec.block = block;
    a.rec[atomicAdd(a.n_rec, 1u)] = rec;
}

// ---------------------------------------------------------------------------------------------------------------- host

using namespace vc_dev;

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// the runs of equal keys of a sorted array: id[i] (1-based) and start[runs + 1]; returns the number of runs, or -1
int64_t run_bounds(DevMem& m, const uint64_t* key, uint32_t n, uint32_t** id_out, uint32_t** start_out) {
    uint32_t *flag = nullptr, *id = nullptr, *start = nullptr;
    if (!m.alloc(&flag, n) || !m.alloc(&id, n)) return -1;
    hipLaunchKernelGGL(k_ovl_heads, dim3(grid(n)), dim3(256), 0, 0, key, n, flag);
    if (!inclusive_sum(m, flag, id, n)) return -1;
    uint32_t runs = 0;
    if (hipMemcpy(&runs, id + (n - 1), 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    m.drop(flag);
    if (!m.alloc(&start, (uint64_t)runs + 1)) return -1;
    hipLaunchKernelGGL(k_ovl_bounds, dim3(grid(n)), dim3(256), 0, 0, key, id, n, start);
    *id_out = id; *start_out = start;
    return runs;
}

// NULL pointers, then the offsets, then the envelope of one set (the callers interleave k / w / limits between the last two)
const char* check_set_ptrs(const vc_overlap_seqs* s) {
    if (!s) return "a sequence set is NULL";
    if (!s->off) return "a sequence set has no offsets";
    return nullptr;
}
const char* check_set_offsets(const vc_overlap_seqs* s) {
    if (s->off[0] != 0) return "offsets do not start at 0";
    for (uint64_t i = 0; i < s->n; ++i) if (s->off[i + 1] < s->off[i]) return "offsets decrease";
    if (s->off[s->n] != 0 && !s->bases) return "a sequence set has bases by its offsets but no base array";
    return nullptr;
}
const char* check_set_envelope(const vc_overlap_seqs* s) {
    if (s->n > VC_OVL_MAX_SEQS) return "more sequences in a set than the envelope (VC_OVL_MAX_SEQS)";
    for (uint64_t i = 0; i < s->n; ++i) if (s->off[i + 1] - s->off[i] > VC_OVL_MAX_LEN) return "a sequence longer than the envelope (VC_OVL_MAX_LEN)";
    return nullptr;
}

// The minimizer table of up to two sets on the device, sequence ids running through both
struct Table {
    uint64_t n = 0;                   // entries
    uint64_t n_seqs = 0;
    uint64_t* hash = nullptr; uint32_t* seq = nullptr; uint32_t* pos = nullptr; uint8_t* strand = nullptr;
    uint64_t* off = nullptr;          // [n_seqs + 1] device
    std::vector<uint64_t> first;      // [n_seqs + 1] host: the first entry of a sequence
};

int sketch(DevMem& m, const vc_overlap_seqs* a, const vc_overlap_seqs* b /* may be NULL */, int k, int w, Table& t) {
    const vc_overlap_seqs* sets[2] = {a, b};
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> blk_seq, blk_start;
    std::vector<uint64_t> first_blk;
    for (const vc_overlap_seqs* s : sets) {
        if (!s) continue;
        const uint64_t base = off.back();
        for (uint64_t i = 0; i < s->n; ++i) {
            const uint64_t len = s->off[i + 1] - s->off[i];
            first_blk.push_back(blk_seq.size());
            for (uint64_t st = 0; st < len; st += kStretch) { blk_seq.push_back((uint32_t)(off.size() - 1)); blk_start.push_back((uint32_t)st); }
            off.push_back(base + s->off[i + 1]);
        }
    }
    first_blk.push_back(blk_seq.size());
    t.n_seqs = off.size() - 1;
    const uint64_t nb = blk_seq.size();
    if (nb >= (1ull << 31)) return fail(VC_ERR_ARG, "more bases than the envelope (2^31 stretches of 256)");
    uint8_t* d_bases = nullptr;
    uint32_t *d_bs = nullptr, *d_bst = nullptr;
    uint64_t *d_cnt = nullptr, *d_boff = nullptr;
    if (!m.alloc(&d_bases, off.back()) || !m.alloc(&t.off, off.size()) || !m.alloc(&d_bs, nb) || !m.alloc(&d_bst, nb) || !m.alloc(&d_cnt, nb) || !m.alloc(&d_boff, nb))
        return fail(VC_ERR_HIP, "hipMalloc failed (sketch)");
    uint64_t at = 0;
    for (const vc_overlap_seqs* s : sets) {
        if (!s || s->off[s->n] == 0) continue;
        if (!to_device(d_bases + at, s->bases, s->off[s->n])) return fail(VC_ERR_HIP, "upload failed (sketch)");
        at += s->off[s->n];
    }
    if (!to_device(t.off, off.data(), off.size())) return fail(VC_ERR_HIP, "upload failed (sketch)");
    t.first.assign(t.n_seqs + 1, 0);
    if (nb == 0) return VC_OK;
    if (!to_device(d_bs, blk_seq.data(), nb) || !to_device(d_bst, blk_start.data(), nb)) return fail(VC_ERR_HIP, "upload failed (sketch)");
    SketchArgs sa{};
    sa.n_blocks = (uint32_t)nb; sa.k = k; sa.w = w; sa.write = 0; sa.blk_seq = d_bs; sa.blk_start = d_bst; sa.off = t.off; sa.bases = d_bases;
    sa.blk_cnt = d_cnt; sa.blk_off = d_boff;
    hipLaunchKernelGGL(k_ovl_sketch, dim3((uint32_t)nb), dim3(kStretch), 0, 0, sa);
    if (!exclusive_sum(m, d_cnt, d_boff, nb)) return fail(VC_ERR_HIP, "scan failed (sketch)");
    std::vector<uint64_t> boff(nb + 1);
    uint64_t last_cnt = 0;
    if (!to_host(boff.data(), d_boff, nb) || !to_host(&last_cnt, d_cnt + (nb - 1), 1)) return fail(VC_ERR_HIP, "sketch kernel failed");
    boff[nb] = boff[nb - 1] + last_cnt;
    t.n = boff[nb];
    if (t.n >= (1ull << 31)) return fail(VC_ERR_HIP, "more minimizers than the envelope (2^31 entries per call)");
    for (uint64_t g = 0; g <= t.n_seqs; ++g) t.first[g] = boff[first_blk[g]];
    if (!m.alloc(&t.hash, t.n) || !m.alloc(&t.seq, t.n) || !m.alloc(&t.pos, t.n) || !m.alloc(&t.strand, t.n)) return fail(VC_ERR_HIP, "hipMalloc failed (minimizer table)");
    sa.write = 1; sa.hash = t.hash; sa.seq = t.seq; sa.pos = t.pos; sa.strand = t.strand;
    hipLaunchKernelGGL(k_ovl_sketch, dim3((uint32_t)nb), dim3(kStretch), 0, 0, sa);
    if (!ran()) return fail(VC_ERR_HIP, "sketch kernel failed");
    m.drop(d_cnt); m.drop(d_boff); m.drop(d_bs); m.drop(d_bst); m.drop(d_bases);
    return VC_OK;
}

// what the library owns between calls (one set per process, like the vc_poa_*_out arrays)
struct Owned {
    std::vector<uint32_t> q_id, t_id, q_begin, q_end, t_begin, t_end, n_anchors, matches, block;
    std::vector<int32_t> score;
    std::vector<uint8_t> strand;
    std::vector<uint64_t> s_hash; std::vector<uint32_t> s_seq, s_pos; std::vector<uint8_t> s_strand;
};
Owned g_own;

constexpr uint64_t kBytesPerAnchor = 56;      // two key arrays, twice (the sort's other side), f, pred, run flag and id

}  // namespace

extern "C" {

const char* vc_overlap_last_error(void) { return g_err.c_str(); }

void vc_overlap_release(void) { g_own = Owned{}; }

void vc_overlap_default_params(vc_overlap_params* p) {
    if (!p) return;
    p->device = 0; p->k = 15; p->w = 5; p->max_occ = 100; p->max_gap = 5000; p->bandwidth = 500; p->lookback = 64;
    p->min_chain_score = 40; p->min_anchors = 3; p->min_overlap = 500; p->drop_internal = 1; p->same_set = 0;
}

int vc_overlap_sketch(int32_t device, int32_t k, int32_t w, const vc_overlap_seqs* s, vc_overlap_sketch_out* o) {
    if (o) std::memset(o, 0, sizeof *o);
    if (!o) return fail(VC_ERR_ARG, "null argument");
    if (const char* e = check_set_ptrs(s)) return fail(VC_ERR_ARG, e);
    if (const char* e = check_set_offsets(s)) return fail(VC_ERR_ARG, e);
    if (k < 4 || k > kMaxK) return fail(VC_ERR_ARG, "k outside 4..28");
    if (w < 1 || w > kMaxW) return fail(VC_ERR_ARG, "w outside 1..64");
    if (const char* e = check_set_envelope(s)) return fail(VC_ERR_ARG, e);
    if (int rc = check_device(device, "the overlapper", g_err)) return rc;
    if (hipSetDevice(device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");
    DevMem m;
    Table t;
    if (int rc = sketch(m, s, nullptr, k, w, t)) return rc;
    if (!to_host(g_own.s_hash, t.hash, t.n) || !to_host(g_own.s_seq, t.seq, t.n) || !to_host(g_own.s_pos, t.pos, t.n) || !to_host(g_own.s_strand, t.strand, t.n))
        return fail(VC_ERR_HIP, "copying the minimizer table failed");
    o->n = t.n; o->hash = g_own.s_hash.data(); o->seq = g_own.s_seq.data(); o->pos = g_own.s_pos.data(); o->strand = g_own.s_strand.data();
    return VC_OK;
}

int vc_overlap(const vc_overlap_params* p, const vc_overlap_seqs* targets, const vc_overlap_seqs* queries, vc_overlap_out* out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!p || !out) return fail(VC_ERR_ARG, "null argument");
    const bool same = p->same_set == 1;
    if (const char* e = check_set_ptrs(targets)) return fail(VC_ERR_ARG, e);
    if (!same) if (const char* e = check_set_ptrs(queries)) return fail(VC_ERR_ARG, e);
    if (const char* e = check_set_offsets(targets)) return fail(VC_ERR_ARG, e);
    if (!same) if (const char* e = check_set_offsets(queries)) return fail(VC_ERR_ARG, e);
    if (p->k < 4 || p->k > kMaxK) return fail(VC_ERR_ARG, "k outside 4..28");
    if (p->w < 1 || p->w > kMaxW) return fail(VC_ERR_ARG, "w outside 1..64");
    if (p->lookback != 64) return fail(VC_ERR_ARG, "lookback is fixed at 64");
    if (p->max_occ <= 0 || p->max_gap <= 0 || p->bandwidth <= 0 || p->min_chain_score <= 0 || p->min_anchors <= 0 || p->min_overlap <= 0)
        return fail(VC_ERR_ARG, "a limit is zero or negative");
    if ((p->drop_internal != 0 && p->drop_internal != 1) || (p->same_set != 0 && p->same_set != 1)) return fail(VC_ERR_ARG, "drop_internal and same_set are 0 or 1");
    if (p->max_occ > VC_OVL_MAX_OCC || p->max_gap > VC_OVL_MAX_GAP || p->bandwidth > VC_OVL_MAX_GAP) return fail(VC_ERR_ARG, "a limit beyond the envelope (VC_OVL_MAX_OCC, VC_OVL_MAX_GAP)");
    if (const char* e = check_set_envelope(targets)) return fail(VC_ERR_ARG, e);
    if (!same) if (const char* e = check_set_envelope(queries)) return fail(VC_ERR_ARG, e);
    if (int rc = check_device(p->device, "the overlapper", g_err)) return rc;
    if (hipSetDevice(p->device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");

    const bool log = getenv("VC_OVL_LOG") != nullptr;
    DevMem m;
    Table t;
    if (int rc = sketch(m, targets, same ? nullptr : queries, p->k, p->w, t)) return rc;
    std::vector<OvlRec> recs;
    const uint32_t n = (uint32_t)t.n, n_targets = (uint32_t)targets->n;
    const uint32_t n_t = (uint32_t)t.first[n_targets];            // entries in the target role (all of them with same_set)
    if (n && n_t) {
        // by hash, stable: a bucket keeps its entries in (set, sequence, position) order
        uint64_t* hs = nullptr;
        uint32_t *iota = nullptr, *perm = nullptr, *bid = nullptr, *bstart = nullptr;
        if (!m.alloc(&hs, n) || !m.alloc(&iota, n) || !m.alloc(&perm, n)) return fail(VC_ERR_HIP, "hipMalloc failed (seeds)");
        hipLaunchKernelGGL(k_ovl_iota, dim3(grid(n)), dim3(256), 0, 0, iota, n);
        if (!sort_pairs(m, t.hash, hs, iota, perm, n, 2 * p->k)) return fail(VC_ERR_HIP, "radix sort failed (seeds)");
        m.drop(iota);
        if (run_bounds(m, hs, n, &bid, &bstart) < 0) return fail(VC_ERR_HIP, "bucket bounds failed");
        SeedArgs sa{};
        sa.n = n; sa.n_t = n_t; sa.same_set = same; sa.max_occ = p->max_occ; sa.k = p->k; sa.perm = perm; sa.bid = bid; sa.bstart = bstart;
        sa.seq = t.seq; sa.pos = t.pos; sa.strand = t.strand; sa.off = t.off; sa.n_targets = n_targets;
        uint64_t* cum = nullptr;
        if (!m.alloc(&sa.cnt, n_t) || !m.alloc(&sa.lo, n_t) || !m.alloc(&sa.hi, n_t) || !m.alloc(&cum, n_t)) return fail(VC_ERR_HIP, "hipMalloc failed (seeds)");
        hipLaunchKernelGGL(k_ovl_count, dim3(grid(n)), dim3(256), 0, 0, sa);
        if (!exclusive_sum(m, sa.cnt, cum, n_t)) return fail(VC_ERR_HIP, "scan failed (seeds)");
        m.drop(hs);
        sa.cum = cum;
        uint64_t total = 0, last_cnt = 0;
        if (hipMemcpy(&total, cum + (n_t - 1), 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&last_cnt, sa.cnt + (n_t - 1), 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(VC_ERR_HIP, "seed kernels failed");
        total += last_cnt;
        // anchors in front of every target: the scan read at the first entry of each
        std::vector<uint64_t> before(n_targets + 1);
        {
            uint64_t *d_idx = nullptr, *d_out = nullptr;
            if (!m.alloc(&d_idx, (uint64_t)n_targets + 1) || !m.alloc(&d_out, (uint64_t)n_targets + 1)) return fail(VC_ERR_HIP, "hipMalloc failed (seeds)");
            if (!to_device(d_idx, t.first.data(), (uint64_t)n_targets + 1)) return fail(VC_ERR_HIP, "upload failed (seeds)");
            hipLaunchKernelGGL(k_ovl_gather, dim3(grid((uint64_t)n_targets + 1)), dim3(256), 0, 0, cum, (uint64_t)n_t, total, d_idx, n_targets + 1, d_out);
            if (hipMemcpy(before.data(), d_out, ((size_t)n_targets + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(VC_ERR_HIP, "seed kernels failed");
            m.drop(d_idx); m.drop(d_out);
        }
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        const uint64_t knob = env_mib("VC_OVL_BUDGET_MB");
        const uint64_t budget = knob ? knob : (uint64_t)(free_b * 0.5);
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(budget / kBytesPerAnchor, 1), (1ull << 31) - 1);
        for (uint32_t ta = 0; ta < n_targets;) {
            uint32_t tb = ta + 1;                                     // at least one target per piece
            while (tb < n_targets && before[tb + 1] - before[ta] <= cap) ++tb;
            const uint64_t na = before[tb] - before[ta];
            if (na >= (1ull << 31)) return fail(VC_ERR_HIP, "one target alone has more anchors than the envelope (2^31)");
            uint32_t n_keys = 0, n_rec = 0;
            if (na) {
                DevMem pm;
                uint64_t *khi = nullptr, *klo = nullptr, *khi2 = nullptr, *klo2 = nullptr;
                if (!pm.alloc(&khi, na) || !pm.alloc(&klo, na) || !pm.alloc(&khi2, na) || !pm.alloc(&klo2, na)) return fail(VC_ERR_HIP, "hipMalloc failed (anchors; lower VC_OVL_BUDGET_MB?)");
                sa.e0 = (uint32_t)t.first[ta]; sa.e1 = (uint32_t)t.first[tb]; sa.khi = khi; sa.klo = klo;
                hipLaunchKernelGGL(k_ovl_emit, dim3(grid(sa.e1 - sa.e0)), dim3(256), 0, 0, sa);
                // by (t_pos, q_pos), then stable by (t_id, q_id, strand)
                if (!sort_pairs(pm, klo, klo2, khi, khi2, (uint32_t)na, 64) || !sort_pairs(pm, khi2, khi, klo2, klo, (uint32_t)na, 64)) return fail(VC_ERR_HIP, "radix sort failed (anchors)");
                pm.drop(khi2); pm.drop(klo2);
                uint32_t *kid = nullptr, *kstart = nullptr;
                const int64_t nk = run_bounds(pm, khi, (uint32_t)na, &kid, &kstart);
                if (nk < 0) return fail(VC_ERR_HIP, "key bounds failed");
                n_keys = (uint32_t)nk;
                pm.drop(kid);
                ChainArgs ca{};
                ca.n_keys = n_keys; ca.kstart = kstart; ca.khi = khi; ca.klo = klo;
                ca.k = p->k; ca.max_gap = p->max_gap; ca.bandwidth = p->bandwidth; ca.min_chain_score = p->min_chain_score; ca.min_anchors = p->min_anchors;
                ca.min_overlap = p->min_overlap; ca.drop_internal = p->drop_internal; ca.same_set = same; ca.off = t.off; ca.n_targets = n_targets;
                if (!pm.alloc(&ca.f, na) || !pm.alloc(&ca.pred, na) || !pm.alloc(&ca.rec, n_keys) || !pm.alloc(&ca.n_rec, 1)) return fail(VC_ERR_HIP, "hipMalloc failed (chains)");
                (void)hipMemset(ca.n_rec, 0, 4);
                hipLaunchKernelGGL(k_ovl_chain, dim3(n_keys), dim3(64), 0, 0, ca);
                if (!ran()) return fail(VC_ERR_HIP, "overlap kernels failed");
                if (hipMemcpy(&n_rec, ca.n_rec, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(VC_ERR_HIP, "overlap kernels failed");
                const size_t had = recs.size();
                recs.resize(had + n_rec);
                if (n_rec && hipMemcpy(recs.data() + had, ca.rec, (size_t)n_rec * sizeof(OvlRec), hipMemcpyDeviceToHost) != hipSuccess) return fail(VC_ERR_HIP, "copying the records failed");
            }
            out->n_keys_total += n_keys;
            if (log) fprintf(stderr, "vc_overlap: piece first=%u targets=%u anchors=%llu keys=%u records=%u\n", ta, tb - ta, (unsigned long long)na, n_keys, n_rec);
            ta = tb;
        }
        out->n_anchors_total = total;
    }
    // one order whatever the pieces and the arrival order of the chains were: a key gives at most one record
    std::sort(recs.begin(), recs.end(), [](const OvlRec& a, const OvlRec& b) {
        if (a.q_id != b.q_id) return a.q_id < b.q_id;
        if (a.t_id != b.t_id) return a.t_id < b.t_id;
        return a.strand < b.strand;
    });
    const size_t nr = recs.size();
    Owned& g = g_own;
    g.q_id.resize(nr); g.t_id.resize(nr); g.strand.resize(nr); g.q_begin.resize(nr); g.q_end.resize(nr); g.t_begin.resize(nr); g.t_end.resize(nr);
    g.n_anchors.resize(nr); g.score.resize(nr); g.matches.resize(nr); g.block.resize(nr);
    for (size_t i = 0; i < nr; ++i) {
        const OvlRec& r = recs[i];
        g.q_id[i] = (uint32_t)r.q_id; g.t_id[i] = (uint32_t)r.t_id; g.strand[i] = (uint8_t)r.strand;
        g.q_begin[i] = (uint32_t)r.q_begin; g.q_end[i] = (uint32_t)r.q_end; g.t_begin[i] = (uint32_t)r.t_begin; g.t_end[i] = (uint32_t)r.t_end;
        g.n_anchors[i] = (uint32_t)r.n_anchors; g.score[i] = r.score; g.matches[i] = (uint32_t)r.matches; g.block[i] = (uint32_t)r.block;
    }
    out->n = nr; out->n_minimizers = t.n;
    out->q_id = g.q_id.data(); out->t_id = g.t_id.data(); out->strand = g.strand.data();
    out->q_begin = g.q_begin.data(); out->q_end = g.q_end.data(); out->t_begin = g.t_begin.data(); out->t_end = g.t_end.data();
    out->n_anchors = g.n_anchors.data(); out->score = g.score.data(); out->matches = g.matches.data(); out->block = g.block.data();
    return VC_OK;
}

}  // extern "C"
