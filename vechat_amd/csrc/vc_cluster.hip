// Clustering of reads into POA groups on the device: overlap records go in, the read groups that vc_poa_run and its kin start
// from come out -- connected components of the qualified overlaps with the strand of every read, filtered by size, numbered
// and ordered.  The reference has no clusterer, so, like vc_overlap.hip and vc_scrub.hip, the library fixes its OWN rule -- all
// integer, every tie decided, written out in include/vechat_hip.h -- and tests/cluster_ref.py restates it with another algorithm
// (a breadth-first search) without sharing a line with this file; tests/test_cluster_gpu.py compares the two array for array.
//
// Test knob, read with getenv on every call:
//   VC_CLUSTER_LOG       set: one line per call on stderr, "vc_cluster: records=M links=L rounds=R components=C kept=K"
//
// Kernels (gfx950, wave64); no thread, wave or block ever waits for another:
//   k_cl_links      one thread per record: the link test -> a flag; after the exclusive scan of the flags the same kernel writes
//                   the two node pairs of every link, (2a, 2b + s) and (2a + 1, 2b + 1 - s), into the compacted edge list
//   k_cl_hook       one thread per edge, one launch: lock-free union by atomicMin on parent[], parent[v] <= v at all times.  find
//                   both ends, hook the larger root under the smaller; an atomicMin that did not meet a root hands back the
//                   parent it met, and the thread goes on with that pair.  The loop's termination argument stands at the loop.
//   k_cl_flatten    one thread per node: parent[v] = the root of v, which is the smallest node of its component -- label(v)
//   k_cl_reads      one thread per read: label(2r), label(2r + 1) -> root, strand, twisted, and the read's sort value and key
//   k_cl_heads      the reads sorted by (root, member key): a flag where a root begins; k_cl_starts, k_cl_sizes, k_cl_kept,
//                   k_cl_number, k_cl_members: the bounds, sizes, the min_size filter, the final numbering and the tables --
//                   flag, scan, write, as in the overlapper and the scrubber
//
// Host: vc_cluster() is the argument checks and three stages -- cl_edges, cl_labels, cl_groups.  DevMem, the checked copies and the
// device check are vc_devutil.h's, the sorts and the sums vc_devscan.h's.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vechat_hip.h"

#include "vc_devscan.h"

namespace {

using namespace vc_dev;

struct LinkArgs {
    uint64_t m; uint64_t min_overlap, cover, identity; int both, write;
    const uint32_t* len;                                   // [n]
    const uint32_t *q_id, *t_id, *q_begin, *q_end, *t_begin, *t_end, *matches, *block;     // [m]
    const uint8_t* strand;
    uint32_t* flag; const uint32_t* idx;                   // [m + 1]: the flags (a 0 at the end) and their exclusive scan
    uint32_t *eu, *ev;                                     // [2 * links]
};

__global__ void k_cl_links(LinkArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t qa = a.q_id[i], tb = a.t_id[i];
    const uint64_t block = a.block[i];
    const bool ca = 1000ull * (a.q_end[i] - a.q_begin[i]) >= a.cover * a.len[qa];
    const bool cb = 1000ull * (a.t_end[i] - a.t_begin[i]) >= a.cover * a.len[tb];
    const bool link = qa != tb && block >= a.min_overlap && (a.identity == 0 || 1000ull * a.matches[i] >= a.identity * block) &&
                      (a.both ? ca && cb : ca || cb);
    if (!a.write) { a.flag[i] = link ? 1u : 0u; return; }
    if (!link) return;
    const uint64_t e = 2ull * a.idx[i];
    const uint32_t s = a.strand[i];
    a.eu[e] = 2 * qa;         a.ev[e] = 2 * tb + s;
    a.eu[e + 1] = 2 * qa + 1; a.ev[e + 1] = 2 * tb + 1 - s;
}

__global__ void k_cl_init(uint64_t n2, uint32_t* parent) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n2) parent[v] = (uint32_t)v;
}

// parent[] as the whole device sees it now: another block's atomicMin is not waited for, but it is not read from a stale line either
__device__ __forceinline__ uint32_t cl_parent(const uint32_t* parent, uint32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A root above v (parent[x] == x when it was read), splitting the path on the way.  parent[x] < x for every x that is not a root,
// so the walk goes strictly down and ends after at most v steps whatever the other threads do; parent[] only ever takes values
// that atomicMin lowers it to, so parent[x] <= x holds at all times.
__device__ __forceinline__ uint32_t cl_find(uint32_t* parent, uint32_t v) {
    uint32_t p = cl_parent(parent, v);
    while (p != v) {
        const uint32_t g = cl_parent(parent, p);
        if (g != p) atomicMin(parent + v, g);                // g < p < v: v's grandparent is a shorter way up
        v = p; p = g;
    }
    return v;
}

__global__ void k_cl_hook(uint64_t n_edges, const uint32_t* eu, const uint32_t* ev, uint32_t* parent) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    uint32_t u = eu[e], v = ev[e];
    // The thread owes the union of u and v.  An entry of parent[] that is replaced, x -> old by x -> lo, never loses a connection:
    // the thread that replaced it goes on owing the union of old and lo.
    // Termination: nothing here waits.  Every pass either ends the loop or goes on with the pair (old, lo), and old < hi and
    // lo < hi, so the larger of the pair falls with every pass: at most hi passes, hi < 2 n.  A pass is repeated only when
    // atomicMin found old != hi, and cl_find had read parent[hi] == hi: that entry has decreased in between.
    for (;;) {
        u = cl_find(parent, u);
        v = cl_find(parent, v);
        if (u == v) break;
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) break;                                // hi was a root and hangs under lo now
        u = old; v = lo;
    }
}

// after the hook launch parent[] is final but for its depth: the root of a tree is the smallest node of the component.  A
// neighbour's entry is either its old parent or its root, both above it in the same tree, so the plain stores race harmlessly.
__global__ void k_cl_flatten(uint64_t n2, uint32_t* parent) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    uint32_t v = (uint32_t)i, p = parent[v];
    while (p != v) { v = p; p = parent[v]; }                 // strictly down: at most i steps
    parent[i] = v;
}

__global__ void k_cl_reads(uint64_t n, const uint32_t* label, const uint32_t* len, uint32_t* root, uint8_t* strand, uint8_t* twisted,
                           uint32_t* idx, uint32_t* key) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t l0 = label[2 * r], l1 = label[2 * r + 1];
    root[r] = l0 >> 1; strand[r] = (uint8_t)(l0 & 1); twisted[r] = l0 == l1 ? 1 : 0;
    idx[r] = (uint32_t)r;
    if (key) key[r] = ~len[r];                               // longest first
}

__global__ void k_cl_gather(uint64_t n, const uint32_t* idx, const uint32_t* root, uint32_t* key) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = root[idx[i]];
}

// sroot: the roots in sorted order.  flag[i] = 1 where a component begins
__global__ void k_cl_heads(uint64_t n, const uint32_t* sroot, uint32_t* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = i == 0 || sroot[i] != sroot[i - 1] ? 1u : 0u;
}

// cinc: the inclusive scan of the flags, so position i lies in component cinc[i] - 1.  start[n_comp + 1]
__global__ void k_cl_starts(uint64_t n, uint32_t n_comp, const uint32_t* flag, const uint32_t* cinc, uint32_t* start) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) start[cinc[i] - 1] = (uint32_t)i;
    if (i == 0) start[n_comp] = (uint32_t)n;
}

__global__ void k_cl_sizes(uint32_t n_comp, uint32_t min_size, const uint32_t* start, uint32_t* size, uint32_t* keep) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_comp) return;
    const uint32_t s = start[c + 1] - start[c];
    size[c] = s; keep[c] = s >= min_size ? 1u : 0u;
    if (c == 0) keep[n_comp] = 0;
}

// the kept components in the order of their roots: comp[k], and ~size as the key of the by_size sort
__global__ void k_cl_kept(uint32_t n_comp, const uint32_t* keep, const uint32_t* kidx, const uint32_t* size, uint32_t* comp, uint32_t* key) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_comp || !keep[c]) return;
    comp[kidx[c]] = (uint32_t)c; key[kidx[c]] = ~size[c];
}

// cluster j is component order[j]: its rank, size, root and twist.  csize[n_kept + 1] with a 0 at the end
__global__ void k_cl_number(uint32_t n_kept, const uint32_t* order, const uint32_t* size, const uint32_t* start, const uint32_t* sroot,
                            const uint8_t* twisted, uint32_t* rank, uint64_t* csize, uint32_t* cl_root, uint8_t* cl_twisted) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_kept) return;
    const uint32_t c = order[j], root = sroot[start[c]];
    rank[c] = (uint32_t)j; csize[j] = size[c]; cl_root[j] = root; cl_twisted[j] = twisted[root];
    if (j == 0) csize[n_kept] = 0;
}

__global__ void k_cl_members(uint64_t n, const uint32_t* cinc, const uint32_t* keep, const uint32_t* rank, const uint32_t* start,
                             const uint64_t* cl_off, const uint32_t* sread, uint32_t* members, uint32_t* cluster) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cinc[i] - 1, r = sread[i];
    if (!keep[c]) { cluster[r] = VC_CLUSTER_NONE; return; }
    const uint32_t j = rank[c];
    members[cl_off[j] + (i - start[c])] = r;                 // the sorted order inside the component is the member order
    cluster[r] = j;
}

// ---------------------------------------------------------------------------------------------------------------- host

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// what the library owns between calls (one set per process, like the vc_scrub_out arrays)
struct Owned {
    std::vector<uint64_t> cl_off;
    std::vector<uint32_t> members, cl_root, cluster;
    std::vector<uint8_t> cl_twisted, strand;
};
Owned g_own;

const char* check_args(const vc_cluster_params* p, const vc_cluster_in* in) {
    if (!in->len && in->n) return "NULL argument: reads without lengths";
    if (in->m && (!in->q_id || !in->t_id || !in->strand || !in->q_begin || !in->q_end || !in->t_begin || !in->t_end || !in->matches || !in->block))
        return "NULL argument: records without an array";
    if (p->min_overlap < 0) return "min_overlap below 0";
    if (p->min_cover_permille < 0 || p->min_cover_permille > 1000) return "min_cover_permille outside 0..1000";
    if (p->cover_both != 0 && p->cover_both != 1) return "cover_both other than 0 / 1";
    if (p->min_identity_permille < 0 || p->min_identity_permille > 1000) return "min_identity_permille outside 0..1000";
    if (p->min_size < 1) return "min_size below 1";
    if (p->by_size != 0 && p->by_size != 1) return "by_size other than 0 / 1";
    if (p->longest_first != 0 && p->longest_first != 1) return "longest_first other than 0 / 1";
    for (uint64_t i = 0; i < in->m; ++i) {
        if (in->q_id[i] >= in->n || in->t_id[i] >= in->n) return "a record of a read that is not there";
        if (in->q_begin[i] >= in->q_end[i] || in->t_begin[i] >= in->t_end[i]) return "a record with an interval that is empty";
        if (in->q_end[i] > in->len[in->q_id[i]] || in->t_end[i] > in->len[in->t_id[i]]) return "a record with an interval outside its read";
        if (in->strand[i] > 1) return "a record with a strand other than 0 / 1";
    }
    if (in->n > VC_CLUSTER_MAX_READS) return "more reads than the envelope (VC_CLUSTER_MAX_READS)";
    for (uint64_t r = 0; r < in->n; ++r) if (in->len[r] > VC_OVL_MAX_LEN) return "a read longer than the envelope (VC_OVL_MAX_LEN)";
    if (in->m >= (1ull << 30)) return "more records than the envelope (m < 2^30)";
    return nullptr;
}

// The device arrays that cross the stages below, and their counts.  Every stage takes the DevMem that its results go into and
// keeps its scratch in one of its own; it returns VC_OK or the code of fail().
struct Cl {
    uint64_t n = 0, m = 0;
    const vc_cluster_params* p = nullptr;
    uint32_t* len = nullptr;                                                      // [n], the whole call
    uint64_t n_links = 0, n_rounds = 0; uint32_t *eu = nullptr, *ev = nullptr;    // edges -> labels
    uint32_t* label = nullptr;                                                    // [2 n] labels -> groups
    uint64_t n_comp = 0, n_kept = 0;
};

// stage 1: records -> the compacted edge list
int cl_edges(DevMem& out, const vc_cluster_in* in, Cl& s) {
    const uint64_t m = s.m;
    if (m == 0) return VC_OK;
    DevMem dm;
    LinkArgs a{};
    uint32_t* idx = nullptr;
    a.m = m; a.min_overlap = (uint64_t)s.p->min_overlap; a.cover = (uint64_t)s.p->min_cover_permille; a.identity = (uint64_t)s.p->min_identity_permille;
    a.both = s.p->cover_both; a.len = s.len;
    if (!dm.alloc(&a.q_id, m, in->q_id) || !dm.alloc(&a.t_id, m, in->t_id) || !dm.alloc(&a.strand, m, in->strand) || !dm.alloc(&a.q_begin, m, in->q_begin) ||
        !dm.alloc(&a.q_end, m, in->q_end) || !dm.alloc(&a.t_begin, m, in->t_begin) || !dm.alloc(&a.t_end, m, in->t_end) ||
        !dm.alloc(&a.matches, m, in->matches) || !dm.alloc(&a.block, m, in->block))
        return fail(VC_ERR_HIP, "hipMalloc or upload failed (records)");
    if (!dm.alloc(&a.flag, m + 1) || !dm.alloc(&idx, m + 1)) return fail(VC_ERR_HIP, "hipMalloc failed (link flags)");
    (void)hipMemset(a.flag + m, 0, 4);
    hipLaunchKernelGGL(k_cl_links, dim3(grid(m)), dim3(256), 0, 0, a);
    if (!exclusive_sum(dm, a.flag, idx, m + 1)) return fail(VC_ERR_HIP, "scan failed (links)");
    uint32_t l32 = 0;
    if (!to_host(&l32, idx + m, 1)) return fail(VC_ERR_HIP, "link kernel failed");
    s.n_links = l32;
    if (s.n_links == 0) return VC_OK;
    if (!out.alloc(&s.eu, 2 * s.n_links) || !out.alloc(&s.ev, 2 * s.n_links)) return fail(VC_ERR_HIP, "hipMalloc failed (edges)");
    a.idx = idx; a.eu = s.eu; a.ev = s.ev; a.write = 1;
    hipLaunchKernelGGL(k_cl_links, dim3(grid(m)), dim3(256), 0, 0, a);
    return ran() ? VC_OK : fail(VC_ERR_HIP, "link kernel failed");              // the records and flags go now: the launch must be through with them
}

// stage 2: edges -> label(v) for the 2 n nodes
int cl_labels(DevMem& out, Cl& s) {
    const uint64_t n2 = 2 * s.n;
    if (!out.alloc(&s.label, n2)) return fail(VC_ERR_HIP, "hipMalloc failed (labels)");
    hipLaunchKernelGGL(k_cl_init, dim3(grid(n2)), dim3(256), 0, 0, n2, s.label);
    if (s.n_links) {
        hipLaunchKernelGGL(k_cl_hook, dim3(grid(2 * s.n_links)), dim3(256), 0, 0, 2 * s.n_links, s.eu, s.ev, s.label);
        hipLaunchKernelGGL(k_cl_flatten, dim3(grid(n2)), dim3(256), 0, 0, n2, s.label);
        s.n_rounds = 1;
    }
    return ran() ? VC_OK : fail(VC_ERR_HIP, "component kernels failed");
}

int bits_of(uint64_t largest) {
    int b = 1;
    while (b < 32 && (largest >> b) != 0) ++b;
    return b;
}

// stage 3: labels -> the tables of the call, on the host
int cl_groups(Cl& s, Owned& g) {
    const uint64_t n = s.n;
    const vc_cluster_params* p = s.p;
    DevMem dm;
    uint32_t *root = nullptr, *idx = nullptr, *idx2 = nullptr, *key = nullptr, *key2 = nullptr, *flag = nullptr, *cinc = nullptr, *start = nullptr;
    uint8_t *strand = nullptr, *twisted = nullptr;
    if (!dm.alloc(&root, n) || !dm.alloc(&strand, n) || !dm.alloc(&twisted, n) || !dm.alloc(&idx, n) || !dm.alloc(&idx2, n) || !dm.alloc(&key, n) || !dm.alloc(&key2, n))
        return fail(VC_ERR_HIP, "hipMalloc failed (reads)");
    hipLaunchKernelGGL(k_cl_reads, dim3(grid(n)), dim3(256), 0, 0, n, s.label, s.len, root, strand, twisted, idx, p->longest_first ? key : nullptr);
    uint32_t* sread = idx;                                                        // the reads by member key: by index as they stand
    if (p->longest_first) {
        if (!sort_pairs(dm, key, key2, idx, idx2, n, 32)) return fail(VC_ERR_HIP, "radix sort failed (lengths)");
        sread = idx2;
    }
    uint32_t* other = sread == idx ? idx2 : idx;
    hipLaunchKernelGGL(k_cl_gather, dim3(grid(n)), dim3(256), 0, 0, n, sread, root, key);
    if (!sort_pairs(dm, key, key2, sread, other, n, bits_of(n - 1))) return fail(VC_ERR_HIP, "radix sort failed (roots)");
    sread = other;
    const uint32_t* sroot = key2;
    // heads and bounds of the components
    if (!dm.alloc(&flag, n) || !dm.alloc(&cinc, n)) return fail(VC_ERR_HIP, "hipMalloc failed (heads)");
    hipLaunchKernelGGL(k_cl_heads, dim3(grid(n)), dim3(256), 0, 0, n, sroot, flag);
    if (!inclusive_sum(dm, flag, cinc, n)) return fail(VC_ERR_HIP, "scan failed (heads)");
    uint32_t c32 = 0;
    if (!to_host(&c32, cinc + (n - 1), 1)) return fail(VC_ERR_HIP, "read kernels failed");
    const uint32_t n_comp = c32;
    s.n_comp = n_comp;
    if (n_comp == 0 || n_comp > n) return fail(VC_ERR_HIP, "read kernels failed: no component");
    uint32_t *size = nullptr, *keep = nullptr, *kidx = nullptr;
    if (!dm.alloc(&start, (uint64_t)n_comp + 1) || !dm.alloc(&size, n_comp) || !dm.alloc(&keep, (uint64_t)n_comp + 1) || !dm.alloc(&kidx, (uint64_t)n_comp + 1))
        return fail(VC_ERR_HIP, "hipMalloc failed (components)");
    hipLaunchKernelGGL(k_cl_starts, dim3(grid(n)), dim3(256), 0, 0, n, n_comp, flag, cinc, start);
    hipLaunchKernelGGL(k_cl_sizes, dim3(grid(n_comp)), dim3(256), 0, 0, n_comp, (uint32_t)p->min_size, start, size, keep);
    if (!exclusive_sum(dm, keep, kidx, (uint64_t)n_comp + 1)) return fail(VC_ERR_HIP, "scan failed (sizes)");
    uint32_t k32 = 0;
    if (!to_host(&k32, kidx + n_comp, 1)) return fail(VC_ERR_HIP, "component kernels failed");
    const uint32_t n_kept = k32;
    s.n_kept = n_kept;
    // the final numbering, the members through it, and cluster[r]
    uint32_t *comp = nullptr, *comp2 = nullptr, *ckey = nullptr, *ckey2 = nullptr, *rank = nullptr, *cl_root = nullptr, *members = nullptr, *cluster = nullptr;
    uint64_t *csize = nullptr, *cl_off = nullptr;
    uint8_t* cl_twisted = nullptr;
    if (!dm.alloc(&comp, n_kept) || !dm.alloc(&comp2, n_kept) || !dm.alloc(&ckey, n_kept) || !dm.alloc(&ckey2, n_kept) || !dm.alloc(&rank, n_comp) ||
        !dm.alloc(&cl_root, n_kept) || !dm.alloc(&cl_twisted, n_kept) || !dm.alloc(&csize, (uint64_t)n_kept + 1) || !dm.alloc(&cl_off, (uint64_t)n_kept + 1) ||
        !dm.alloc(&members, n) || !dm.alloc(&cluster, n))
        return fail(VC_ERR_HIP, "hipMalloc failed (clusters)");
    uint64_t total = 0;
    if (n_kept) {
        hipLaunchKernelGGL(k_cl_kept, dim3(grid(n_comp)), dim3(256), 0, 0, n_comp, keep, kidx, size, comp, ckey);
        const uint32_t* order = comp;
        if (p->by_size) {
            if (!sort_pairs(dm, ckey, ckey2, comp, comp2, n_kept, 32)) return fail(VC_ERR_HIP, "radix sort failed (sizes)");
            order = comp2;
        }
        hipLaunchKernelGGL(k_cl_number, dim3(grid(n_kept)), dim3(256), 0, 0, n_kept, order, size, start, sroot, twisted, rank, csize, cl_root, cl_twisted);
        if (!exclusive_sum(dm, csize, cl_off, (uint64_t)n_kept + 1)) return fail(VC_ERR_HIP, "scan failed (cluster sizes)");
        if (!to_host(&total, cl_off + n_kept, 1)) return fail(VC_ERR_HIP, "cluster kernels failed");
        if (total > n) return fail(VC_ERR_HIP, "cluster kernels failed: more members than reads");
    }
    hipLaunchKernelGGL(k_cl_members, dim3(grid(n)), dim3(256), 0, 0, n, cinc, keep, rank, start, cl_off, sread, members, cluster);
    if (!ran()) return fail(VC_ERR_HIP, "member kernel failed");
    if (n_kept == 0) g.cl_off.assign(1, 0);
    else if (!to_host(g.cl_off, cl_off, (uint64_t)n_kept + 1)) return fail(VC_ERR_HIP, "copying the clusters failed");
    if (!to_host(g.members, members, total) || !to_host(g.cl_root, cl_root, n_kept) || !to_host(g.cl_twisted, cl_twisted, n_kept) ||
        !to_host(g.cluster, cluster, n) || !to_host(g.strand, strand, n))
        return fail(VC_ERR_HIP, "copying the clusters failed");
    return VC_OK;
}

}  // namespace

extern "C" {

const char* vc_cluster_last_error(void) { return g_err.c_str(); }

void vc_cluster_release(void) { g_own = Owned{}; }

void vc_cluster_default_params(vc_cluster_params* p) {
    if (!p) return;
    p->device = 0; p->min_overlap = 500; p->min_cover_permille = 800; p->cover_both = 1; p->min_identity_permille = 0; p->min_size = 2;
    p->by_size = 0; p->longest_first = 0;
}

int vc_cluster(const vc_cluster_params* p, const vc_cluster_in* in, vc_cluster_out* out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!p || !in || !out) return fail(VC_ERR_ARG, "NULL argument");
    if (const char* e = check_args(p, in)) return fail(VC_ERR_ARG, e);
    if (int rc = check_device(p->device, "the clusterer", g_err)) return rc;
    if (hipSetDevice(p->device) != hipSuccess) return fail(VC_ERR_HIP, "hipSetDevice failed");

    Owned& g = g_own;
    Cl s;
    s.n = in->n; s.m = in->m; s.p = p;
    if (s.n == 0) {
        g.members.clear(); g.cl_root.clear(); g.cluster.clear(); g.cl_twisted.clear(); g.strand.clear();
        g.cl_off.assign(1, 0);
    } else {
        DevMem labels;                                       // the lengths and the labels: to the end of the call
        if (!labels.alloc(&s.len, s.n, in->len)) return fail(VC_ERR_HIP, "hipMalloc or upload failed (lengths)");
        {
            DevMem edges;                                    // gone before the reads are sorted
            if (int rc = cl_edges(edges, in, s)) return rc;
            if (int rc = cl_labels(labels, s)) return rc;
        }
        if (int rc = cl_groups(s, g)) return rc;
    }
    if (getenv("VC_CLUSTER_LOG"))
        fprintf(stderr, "vc_cluster: records=%llu links=%llu rounds=%llu components=%llu kept=%llu\n", (unsigned long long)s.m, (unsigned long long)s.n_links,
                (unsigned long long)s.n_rounds, (unsigned long long)s.n_comp, (unsigned long long)s.n_kept);
    // a vector's data() may be NULL when it is empty: every array handed out is a real address
    static const uint32_t none32 = 0;
    static const uint8_t none8 = 0;
    auto p32 = [](const std::vector<uint32_t>& v) { return v.empty() ? &none32 : v.data(); };
    auto p8 = [](const std::vector<uint8_t>& v) { return v.empty() ? &none8 : v.data(); };
    out->n_clusters = s.n_kept; out->cl_off = g.cl_off.data(); out->members = p32(g.members); out->cl_root = p32(g.cl_root);
    out->cl_twisted = p8(g.cl_twisted); out->cluster = p32(g.cluster); out->strand = p8(g.strand);
    out->n_links = s.n_links; out->n_rounds = s.n_rounds; out->n_components = s.n_comp;
    return VC_OK;
}

}  // extern "C"
