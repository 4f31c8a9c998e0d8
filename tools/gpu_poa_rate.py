"""POA-group rate on one MI355X (vc_poa_run, vechat_amd/poa.py), the shape nobody had measured: 4 096 groups of 32 x 1 kb.  Groups come
from vc_synth windows with frac_partial=0 -- the backbone and its 31 layers become one group, in stored order, with their qualities.

For each algorithm (local, global, semi-global) one warm-up call -- on all groups for the first, so that the buffer cache has grown
to the batch, on 64 for the others -- then one timed call on all of them (host clock around
the synchronous call), reported as groups/s and GCUPS with cells = sum over alignments of graph rows x sequence length (the
large path's VC_LARGE_LOG "done" line).  Then, in a run of its own per algorithm, the same call under
`rocprofv3 --kernel-trace --stats` for the time shares of the k_lg_* kernels.  Last, the reference's spoa (oracle/_ref
libvcref_sse41.so, vcref_spoa_consensus) on a sample of the same groups on 16 host threads (ctypes releases the GIL), its consensus
compared with the device's.

  python tools/gpu_poa_rate.py [--groups 4096] [--len 1000] [--depth 32] [--cpu-sample 256] [--out profiles/poa_rate.txt]
                               [--gaps linear|affine|convex] [--msa] [--strand] [--graph [--parent-lib LIB]] [--haplotypes [--parent-lib LIB]]

--msa measures the multiple sequence alignment instead (vc_poa_run_msa with the consensus row and the coverage, global
alignment) and writes profiles/poa_msa_rate.txt: after one warm-up call on all groups, three consensus-only calls and three
MSA calls in the same process, then each kind once under `rocprofv3 --kernel-trace --stats` (kernel trace only) for k_lg_apply's
and k_lg_msa's kernel time -- the label bookkeeping shows as the difference of k_lg_apply between the two traces, and what the
MSA call's wall time exceeds the consensus-only one's beyond the kernels is the copy-out and the host's assembly.

--strand measures the strand-ambiguous call (vc_poa_run_strand, consensus only, global alignment, the gap model of --gaps) and
writes profiles/poa_strand_rate.txt: every second member of every group, never member 0, is reverse-complemented (its quality
string reversed); after one warm-up call, three plain calls (vc_poa_run_msa without flags, which is vc_poa_run_gaps) on the
unflipped groups and three strand calls on the flipped ones in the same process, the number of groups whose consensus differs
between the two (the synthetic reads are upper-case ACGT, so 0 is expected), the members reported reversed, and then each kind
once under `rocprofv3 --kernel-trace --stats` for the k_lg_* shares.  Exits 1 if the strand call takes 2x the plain call's time
or more: two whole flows would cost that, so it would mean the graph stages or the launches were duplicated.

--graph measures the graph output (vc_poa_run_graph, global alignment, 5/-4/-8; profiles/poa_graph_rate.txt): in one process
three consensus-only calls and three graph calls with the bytes copied out; with --parent-lib (a library built from the parent
commit) the consensus-only calls of that library and of this one in alternating processes of their own (parent, this, parent,
this; a warm-up and three timed calls each), for the comparison against the spread of the parent's own runs; then the
graph call under `rocprofv3 --kernel-trace --stats` once per path route (scatter and compaction, and the literal walk of
VC_LARGE_GRAPH_WALK=1) for k_lg_graph's time beside k_lg_msa<1>'s on the same groups.  Exits 1 if the GFA of a sampled group
differs from the one of the CPU restatement tests/poa_graph_ref.py (--check groups, the smallest ones of the batch).

--gaps affine / convex runs vc_poa_run_gaps with spoa's affine known-answer scores (5 -4 -8 -6) or its command-line defaults
(5 -4 -8 -6 -10 -4, convex); the cells are still rows x columns (not x planes).  The reference in oracle/_ref only takes linear
gaps, so those runs have no host comparison.
--align [--queries-per-group 32] [--parent-lib LIB]: the query stage of vc_poa_run_align (profiles/poa_align_rate.txt).  The groups
are built from all members but the last; the last and --queries-per-group mutated members are each group's queries.  Three calls
of each kind after a warm-up in one process: the stage's own time is the call minus the plain call, its GCUPS the rows x length
of the align log line over that time; then the consensus-only rate beside the parent commit's library in alternating processes,
for every gap model of --parent-gaps (the shared row body, a template over the gap model, changes how k_lg_fwd is compiled); then one rocprofv3 --kernel-trace --stats run of its own for the shares of
the query kernels and the cells per forward-kernel second of k_lg_qfwd beside k_lg_fwd.
--resume [--parent-lib LIB]: groups that go on from a stored graph (vc_poa_run_from; profiles/poa_resume_rate.txt), global, 5/-4/-8,
one process, three calls of each kind after a warm-up, the library call alone on the clock (the stored graphs are packed into a
vc_poa_graph_in before it, and nothing is copied out of the library's tables inside it):
  (a) every group built once from all members with its state; then vc_poa_run_from on the stored graphs with no new member and one
      query per group, beside vc_poa_run_align on the same groups and queries.  Expected: the load plus the query stage, a small
      fraction of the rebuild, since the --depth dependent steps of the build are skipped; checked as below a quarter of it;
  (b) the first 3/4 of the members built with their state, then the last quarter added, beside the one-shot build of all, each
      with the graph tables and the state as outputs.  Expected: about a quarter of the build plus the load; checked as below half
      of it (the last members meet the largest graphs, so they cost more than the average member);
  (c) one rocprofv3 --kernel-trace --stats run of its own (build 3/4, add 1/4) for k_lg_load beside k_lg_apply;
  (d) with --parent-lib the consensus-only rate of this library beside the parent commit's in alternating processes.
Exits 1 if a stored-graph result differs from the one-shot one or an expectation of (a) or (b) is missed.
--weights [--parent-lib LIB]: explicit weights and the consensus profile (vc_poa_run_weighted) on the standard groups: the plain path
beside the parent commit's library in alternating processes, every member weighted per base, the profile call beside the consensus
and the MSA call with the bytes each copies out, a traced run -> profiles/poa_weights_rate.txt.
--spans [--groups 512] [--locus 8000] [--len 1000] [--depth 32] [--parent-lib LIB]: span-limited alignment (vc_poa_run_spans;
profiles/poa_spans_rate.txt).  Every group is one random backbone of --locus bases plus locus / len x depth reads of --len bases
tiled over it, their true ranges as spans; global, 5/-4/-8, one process, three calls of each kind after a warm-up: the span call
and the plain call on the same groups, with sub_rows / full_rows of the `spans` log line.  Expected, stated in the file before the
figures: the forward cells fall by about len / locus, k_lg_apply and the serial subgraph() in k_lg_prep do not, so the time falls
by less.  With --parent-lib the plain path -- consensus only on the standard 4 096 groups of 32 x 1 kb -- of this library beside
the parent commit's in alternating processes; then one rocprofv3 --kernel-trace --stats run of its own of the span call for the
shares of k_lg_prep, k_lg_fwd and k_lg_apply.
--assign [--groups 256] [--queries 1024] [--len 1000] [--depth 32]: queries assigned to groups (vc_poa_run_assign;
profiles/poa_assign_rate.txt).  The queries are mutated members of the groups in turn; global, 5/-4/-8, one strand.  The assign
call with the dense table beside the existing route to the same scores -- vc_poa_run_align without pairs on the queries repeated
per group -- in one process on the same pairs, one untimed call of each, then two of each alternating: pairs/s and GCUPS of the
stage (call minus the build alone), forward launches, ring_cells / full_cells of the `assign` log line, sampled scores compared;
then one rocprofv3 --kernel-trace --stats run of its own with one call of each route on a quarter of the pairs for the shares of
k_lg_sfwd, k_lg_qfwd, k_lg_slots and k_lg_assign.  The expectation is stated in the file before the figures.  Exits 1 if the
assign call is slower than the existing route beyond that route's own spread between its two runs.
--haplotypes [--parent-lib LIB]: the haplotype split (vc_poa_run_haplotypes; profiles/poa_haplo_rate.txt) on 4 096 groups of 32 x 1 kb
reads, every second group drawn from two haplotypes (a SNP every 100 bases, half of the reads each), 8 % read errors, FASTA; global,
5/-4/-8, the rule's defaults.  In one process, three calls of each kind after a warm-up: the plain call, the haplotype call and the
graph call, with the bytes each copies out and the haplotype counts found.  With --parent-lib the plain path -- consensus only on
the standard groups -- of this library beside the parent commit's in alternating processes; then one rocprofv3 --kernel-trace
--stats run of its own of the haplotype call for the shares of k_lg_hap and k_lg_hapcons.  The expectation is stated in the file
before the figures.  Nothing is asserted about the new stage's own speed: exits 1 only if the plain path falls outside the
parent's own spread.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from vechat_amd import capi, large, poa  # noqa: E402

NAMES = {0: "local (kSW)", 1: "global (kNW)", 2: "semi-global (kOV)"}
GAPS = {"linear": None, "affine": (-8, -6, -8, -6), "convex": (-8, -6, -10, -4)}    # gap_open, gap_extend, gap_open2, gap_extend2


def params(alg, gaps):
    if GAPS[gaps] is None:
        return capi.VcPoaParams(device=0, algorithm=alg, match=5, mismatch=-4, gap=-8)
    g, e, q, c = GAPS[gaps]
    return capi.VcPoaGapParams(device=0, algorithm=alg, match=5, mismatch=-4, gap_open=g, gap_extend=e, gap_open2=q, gap_extend2=c)


def synth_groups(a):
    cfg = capi.synth_cfg(seed=4100, backbone_len=a.len, n_layers=a.depth - 1, frac_partial=0.0)
    return capi.synth_batch(cfg, 0, a.groups)


def timed(batch, alg, warm, gaps="linear"):
    """-> (seconds, consensus, statuses, alignments, cells) of one vc_poa_run on the batch, VC_LARGE_LOG read from stderr.
    warm: "full" -- one untimed call on the whole batch first, so that the large path's buffer cache has grown to the batch's size
    (the first call of a process allocates it); "small" -- 64 groups (code objects loaded)."""
    p = params(alg, gaps)
    if warm:
        poa.run_batch(batch if warm == "full" else batch.slice(0, min(64, batch.n_windows)), p)
    import tempfile
    with tempfile.TemporaryFile() as log:          # the library's stderr lines, into a file (a pipe could fill and block it)
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            cons, status = poa.run_batch(batch, p)
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read()
    done = [l for l in err.decode().splitlines() if l.startswith("vc_large: done")][-1]
    kv = dict(t.split("=") for t in done.split()[2:])
    return dt, cons, status, int(kv["alignments"]), int(kv["cells"])


def kernel_shares(trace_dir):
    """{kernel: ms} from a rocprofv3 kernel trace"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    ms = defaultdict(float)
    for f in files:
        for row in csv.DictReader(open(f)):
            k = row["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
            k = k.split("::")[-1]
            ms[k] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
    return dict(ms)


def timed_msa(batch, flags):
    """-> (seconds, rows_bytes, alignments, cells) of one vc_poa_run_msa (global, 5/-4/-8 linear) on the batch"""
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    import ctypes as C
    import tempfile
    import numpy as np
    lib = capi.load_hip()
    n = batch.n_windows
    cons, off, status = np.zeros(int(batch.bases.size), np.uint8), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    o = capi.VcPoaMsaOut(flags=flags)
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            rc = lib.vc_poa_run_msa(C.byref(p), C.byref(vb), C.byref(r), C.byref(o))
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if rc != 0 or int((status != 0).sum()):
        raise RuntimeError(f"vc_poa_run_msa: rc {rc}, {int((status != 0).sum())} groups not computed")
    done = [l for l in err.splitlines() if l.startswith("vc_large: done")][-1]
    kv = dict(t.split("=") for t in done.split()[2:])
    return dt, int(o.rows_bytes), int(kv["alignments"]), int(kv["cells"])


def flip_members(batch):
    """every second member of every group, never member 0, reverse-complemented in place of itself (quality reversed)"""
    import numpy as np
    comp = np.arange(256, dtype=np.uint8)
    for x, y in ("AT", "CG", "RY", "KM", "BV", "DH"):
        for u, v in ((x, y), (y, x)):
            comp[ord(u)] = comp[ord(u.lower())] = ord(v)
    comp[ord("U")] = comp[ord("u")] = ord("A")
    bases, quals = batch.bases.copy(), batch.quals.copy()
    flips = np.zeros(batch.n_seqs, bool)
    for w in range(batch.n_windows):
        s0, s1 = int(batch.win_seq_off[w]), int(batch.win_seq_off[w + 1])
        for s in range(s0 + 1, s1, 2):
            o0, o1 = int(batch.seq_off[s]), int(batch.seq_off[s + 1])
            bases[o0:o1] = comp[batch.bases[o0:o1]][::-1]
            quals[o0:o1] = batch.quals[o0:o1][::-1]
            flips[s] = True
    return capi.Batch(batch.win_seq_off, batch.seq_off, batch.seq_begin, batch.seq_end, batch.seq_has_qual, bases, quals,
                      batch.win_fasta), flips


def gap_params(gaps):
    g, e, q, c = GAPS[gaps] or (-8, -8, -8, -8)
    return capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=g, gap_extend=e, gap_open2=q, gap_extend2=c)


def timed_strand(batch, gaps, strand):
    """-> (seconds, consensus per group, reversed per sequence or None, alignments, cells) of one vc_poa_run_strand (strand) or
    vc_poa_run_msa without flags (plain) on the batch, global alignment"""
    import ctypes as C
    import tempfile
    import numpy as np
    lib = capi.load_hip()
    p = gap_params(gaps)
    n = batch.n_windows
    cons, off, status = np.zeros(int(batch.bases.size), np.uint8), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    o = capi.VcPoaMsaOut(flags=0)
    rev = np.zeros(max(batch.n_seqs, 1), np.uint8)
    so = capi.VcPoaStrandOut(rev.ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            if strand:
                rc = lib.vc_poa_run_strand(C.byref(p), C.byref(vb), C.byref(r), C.byref(o), C.byref(so))
            else:
                rc = lib.vc_poa_run_msa(C.byref(p), C.byref(vb), C.byref(r), C.byref(o))
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if rc != 0 or int((status != 0).sum()):
        raise RuntimeError(f"rc {rc}, {int((status != 0).sum())} groups not computed")
    done = [l for l in err.splitlines() if l.startswith("vc_large: done")][-1]
    kv = dict(t.split("=") for t in done.split()[2:])
    return (dt, [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)], rev[:batch.n_seqs].astype(bool) if strand else None,
            int(kv["alignments"]), int(kv["cells"]))


def main_strand(a):
    batch = synth_groups(a)
    fbatch, flips = flip_members(batch)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_strand_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = open(out).read().splitlines() if a.append and os.path.exists(out) else []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    g = GAPS[a.gaps] or (-8,)
    emit(f"POA groups with both strands ({a.gaps} gaps, 5/-4/{'/'.join(map(str, g))}): {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed "
         f"4100, PacBio-like errors, frac_partial=0, FASTQ), {int(batch.seq_off[-1])} bases; global (kNW), consensus only; one MI355X; "
         f"host clock around one synchronous call; one untimed strand call on all groups first, then three plain calls "
         f"(vc_poa_run_msa, flags 0) on the groups as synthesised and three strand calls (vc_poa_run_strand) on the groups with "
         f"every second member, never member 0, reverse-complemented ({int(flips.sum())} of {batch.n_seqs} members), in the same process")
    timed_strand(fbatch, a.gaps, True)
    plain = [timed_strand(batch, a.gaps, False) for _ in range(3)]
    both = [timed_strand(fbatch, a.gaps, True) for _ in range(3)]
    for name, runs in (("plain, unflipped groups", plain), ("both strands, flipped groups", both)):
        emit(f"{name:30s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) + f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in runs)} s; "
             f"{runs[0][3]} alignments, {runs[0][4] / 1e9:.2f} G cells)")
    differ = sum(1 for x, y in zip(plain[0][1], both[0][1]) if x != y)
    wrong = int((both[0][2] != flips).sum())
    mp, mb = min(r[0] for r in plain), min(r[0] for r in both)
    emit(f"groups whose consensus differs between the two: {differ} of {a.groups} (expected 0); members whose reported strand is not "
         f"the flip that was applied: {wrong} of {batch.n_seqs}")
    emit(f"strand / plain time (best of three each): {mb / mp:.3f} (must stay below 2; the forward pass alone doubles)")
    large.release()
    if not a.no_trace:
        emit("kernel time shares, each kind's call in a run of its own under rocprofv3 --kernel-trace --stats (a fresh process: 64 groups first, then all):")
        for kind, flag in (("plain", 0), ("both strands", 1)):
            d = os.path.join(a.trace_dir, f"strand{flag}_{a.gaps}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", str(flag), "--strand", "--groups", str(a.groups), "--len", str(a.len),
                   "--depth", str(a.depth), "--gaps", a.gaps]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"  {kind}: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                break
            ms = kernel_shares(d)
            tot = sum(ms.values())
            shares = ", ".join(f"{k} {v / tot * 100:.1f} % ({v / 1e3:.2f} s)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1]))
            wall = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            emit(f"  {kind:13s} kernels {tot / 1e3:.2f} s of {wall:.2f} s wall: {shares}")
    print("wrote", out)
    return 1 if mb >= 2 * mp else 0


def main_msa(a):
    batch = synth_groups(a)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_msa_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    emit(f"POA groups with the MSA: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like errors, frac_partial=0, FASTQ), "
         f"{int(batch.seq_off[-1])} bases; 5/-4/-8, global (kNW); one MI355X; vc_poa_run_msa, synchronous; host clock around one call; "
         f"one untimed call on all groups first, then three calls of each kind in the same process")
    timed_msa(batch, 0)
    plain = [timed_msa(batch, 0) for _ in range(3)]
    full = [timed_msa(batch, 7) for _ in range(3)]
    for name, runs in (("consensus only (flags 0)", plain), ("MSA + consensus row + coverage (flags 7)", full)):
        emit(f"{name:42s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) + f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in runs)} s; "
             f"{runs[0][2]} alignments, {runs[0][3] / 1e9:.2f} G cells, output blocks {runs[0][1] / 1e6:.1f} MB)")
    mp, mf = min(r[0] for r in plain), min(r[0] for r in full)
    emit(f"MSA / consensus-only rate (best of three each): {mp / mf:.3f}; the MSA call takes {mf - mp:.2f} s longer")
    large.release()
    if a.no_trace:
        return
    emit("kernel times, each kind's call in a run of its own under rocprofv3 --kernel-trace --stats (a fresh process: 64 groups first, then all):")
    traced = {}
    for kind, flags in (("consensus only", 0), ("MSA", 7)):
        d = os.path.join(a.trace_dir, f"msa{flags}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", str(flags), "--msa", "--groups", str(a.groups), "--len", str(a.len),
               "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"  {kind}: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return
        ms = kernel_shares(d)
        traced[flags] = ms
        wall = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
        emit(f"  {kind:15s} kernels {sum(ms.values()) / 1e3:.2f} s of {wall:.2f} s wall: " +
             ", ".join(f"{k} {v / 1e3:.3f} s" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    ap0 = sum(v for k, v in traced[0].items() if k.startswith("k_lg_apply"))
    ap7 = sum(v for k, v in traced[7].items() if k.startswith("k_lg_apply"))
    km = sum(v for k, v in traced[7].items() if k.startswith("k_lg_msa"))
    emit(f"(i) label bookkeeping: k_lg_apply {ap0 / 1e3:.3f} s without, {ap7 / 1e3:.3f} s with labels (+{(ap7 - ap0) / 1e3:.3f} s, the 64-group "
         f"warm-up included in both); (ii) k_lg_msa, both phases: {km / 1e3:.3f} s = {km / ap7 * 100:.2f} % of k_lg_apply's time in the same trace; "
         f"(iii) copy-out and host assembly: what remains of the {mf - mp:.2f} s above, about {mf - mp - (ap7 - ap0 + km) / 1e3:.2f} s "
         f"for {full[0][1] / 1e6:.1f} MB")
    print("wrote", out)


def timed_graph(batch, flags=0, graph=True, lib=None):
    """-> (seconds, bytes copied out, graphs or None) of one vc_poa_run_graph (global, 5/-4/-8 linear; flags: the MSA beside it) on
    the batch, or with graph=False of the consensus-only vc_poa_run_gaps (lib: another library's handle, see parent_handle)"""
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    import re
    import tempfile
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            res, status = poa.run_batch_graph(batch, p, flags) if graph else poa.run_batch(batch, p, lib)
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if int((status != 0).sum()):
        raise RuntimeError(f"{int((status != 0).sum())} groups not computed")
    m = re.search(r"vc_large: graph launches=(\d+) bytes=(\d+)", err)
    return dt, int(m.group(2)) if m else 0, res if graph else None


def parent_handle(path):
    """The two entry points the consensus-only call needs, from a library that may lack the newer ones."""
    import ctypes as C
    return capi.bind(C.CDLL(path), ("vc_poa_run_gaps", "vc_poa_last_error"))


def _gfa_job(args):
    import poa_graph_ref as G
    mem, names = args
    return G.to_poa_graph(G.graph(mem, 1, 5, -4, -8)).to_gfa(names, include_consensus=True)


def main_graph(a):
    batch = synth_groups(a)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_graph_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    emit(f"POA groups with the graph output: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like errors, frac_partial=0, "
         f"FASTQ), {int(batch.seq_off[-1])} bases; 5/-4/-8, global (kNW); one MI355X; synchronous; host clock around one call; one untimed "
         f"call on all groups first, then three calls of each kind in the same process")
    timed_graph(batch, graph=False)
    plain = [timed_graph(batch, graph=False)[0] for _ in range(3)]
    emit(f"{'consensus only (vc_poa_run_gaps)':44s} " + "  ".join(f"{a.groups / t:7.1f}" for t in plain) + f" groups/s  ({'  '.join(f'{t:.2f}' for t in plain)} s)")
    runs = [timed_graph(batch) for _ in range(3)]
    emit(f"{'graph (vc_poa_run_graph, Python copies incl.)':44s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) +
         f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in runs)} s; {runs[0][1] / 1e6:.1f} MB copied out of the device)")
    graphs = runs[-1][2]
    large.release()
    ok = True
    if a.check:
        sizes = [int(batch.seq_off[batch.win_seq_off[w + 1]] - batch.seq_off[batch.win_seq_off[w]]) for w in range(batch.n_windows)]
        idx = sorted(range(batch.n_windows), key=lambda w: sizes[w])[:a.check]
        jobs = []
        for w in idx:
            seqs, quals, _, _ = batch.window(w)
            jobs.append((list(zip(seqs, quals)), [f"r{i}" for i in range(len(seqs))]))
        from concurrent.futures import ProcessPoolExecutor
        with ProcessPoolExecutor(min(a.threads, len(jobs))) as ex:
            want = list(ex.map(_gfa_job, jobs))
        bad = [w for w, (mem, names), t in zip(idx, jobs, want) if graphs[w].to_gfa(names, include_consensus=True) != t]
        ok = not bad
        emit(f"GFA of {len(idx)} sampled groups (the smallest of the batch: {idx}) against the CPU restatement: " +
             ("identical" if ok else f"DIFFERENT for {bad}"))
    del graphs, runs
    if a.parent_lib:
        # the two libraries alternate, each run a process of its own (a warm-up call, then three timed ones): parent, this, parent, this
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "0", "--graph", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            name = "library of the parent commit" if which == "parent" else "this library"
            emit(f"{'consensus only, ' + name:44s} " + "  ".join(f"{a.groups / x:7.1f}" for x in t) +
                 f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        lo, hi = par[0], par[-1]
        med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        emit(f"consensus-only time over the two alternated processes each: the parent's {lo:.3f} .. {hi:.3f} s (its own spread "
             f"{(hi - lo) / lo * 100:.2f} %, median {med(par):.3f}), this library's {cur[0]:.3f} .. {cur[-1]:.3f} s (median {med(cur):.3f}): "
             f"best against best {(cur[0] / lo - 1) * 100:+.2f} %, median against median {(med(cur) / med(par) - 1) * 100:+.2f} %; this "
             f"library's median lies {'inside (or below)' if med(cur) <= hi else 'ABOVE'} the range of the parent's own runs")
    if not a.no_trace:
        emit("kernel times of the graph call (with the MSA beside it, flags 7), a run of its own per path route under rocprofv3 --kernel-trace "
             "--stats (a fresh process: 64 groups first, then all):")
        digests = []
        for route, child_id in (("scatter + compaction", 1), ("literal walk", 2)):
            d = os.path.join(a.trace_dir, f"graph{child_id}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", str(child_id), "--graph", "--groups", str(a.groups), "--len", str(a.len),
                   "--depth", str(a.depth)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"  {route}: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1
            ms = kernel_shares(d)
            tot = sum(ms.values())
            kg = {k: v for k, v in ms.items() if k.startswith("k_lg_graph") or k.startswith("k_lg_msa")}
            emit(f"  {route:21s} kernels {tot / 1e3:.2f} s: " + ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(kg.items())))
            digests.append([json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["paths"])
        if len(digests) == 2:
            same = digests[0] == digests[1]
            ok = ok and same
            emit(f"  the paths of all {a.groups} groups by the two routes: " + ("identical" if same else "DIFFERENT"))
    print("wrote", out)
    return 0 if ok else 1


def align_batches(a, batch):
    """the groups without their last member, and per group that member plus --queries-per-group mutated members as queries"""
    import random
    rng = random.Random(4101)
    groups, queries = [], []
    for w in range(batch.n_windows):
        seqs, quals, _, _ = batch.window(w)
        groups.append(list(zip(seqs[:-1], quals[:-1])))
        qs = [seqs[-1]]
        for _ in range(a.queries_per_group):
            s = bytearray(rng.choice(seqs[:-1]))
            for _ in range(max(1, len(s) // 20)):                      # 5 % substitutions
                s[rng.randrange(len(s))] = rng.choice(b"ACGT")
            qs.append(bytes(s))
        queries.append(qs)
    return poa.group_batch(groups), poa.query_batch(queries)


def timed_align(gb, qb, flags, queries=True):
    """-> (seconds, the align log line's (jobs, launches, cells, bytes) or None) of one vc_poa_run_align (global, 5/-4/-8 linear), or
    with queries=False of the plain vc_poa_run_gaps on the same groups"""
    import re
    import tempfile
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            status = poa.run_batch_align(gb, qb, p, flags)[1] if queries else poa.run_batch(gb, p)[1]
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if int((status != 0).sum()):
        raise RuntimeError(f"{int((status != 0).sum())} groups not computed")
    m = re.search(r"vc_large: align jobs=(\d+) launches=(\d+) cells=(\d+) bytes=(\d+)", err)
    return dt, tuple(map(int, m.groups())) if m else None


def main_align(a):
    """The query stage beside the plain call on the same groups, in one process: its own time is the call minus the plain call;
    then the consensus-only rate beside the parent commit's library (the shared row body changes how k_lg_fwd is compiled), as
    --graph --parent-lib does; then one kernel trace for the shares of the query kernels beside k_lg_fwd."""
    gb, qb = align_batches(a, synth_groups(a))
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_align_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    nq = int(qb.win_seq_off[-1])
    emit(f"queries against finished POA groups: {a.groups} groups of {a.depth - 1} x {a.len} bp (vc_synth seed 4100; the last member of "
         f"{a.depth} held out), {nq} queries ({1 + a.queries_per_group} per group: the held-out member and mutated members); 5/-4/-8, "
         f"global (kNW); one MI355X; synchronous; host clock around one call; one untimed call first, then three of each kind")
    timed_align(gb, qb, 1)
    plain = [timed_align(gb, qb, 0, queries=False)[0] for _ in range(3)]
    emit(f"{'plain (vc_poa_run_gaps)':40s} " + "  ".join(f"{t:.3f}" for t in plain) + " s")
    base = sorted(plain)[1]
    for name, flags in (("scores only", 0), ("pairs", 1), ("pairs, both strands", 3)):
        runs = [timed_align(gb, qb, flags) for _ in range(3)]
        stage = [max(r[0] - base, 1e-9) for r in runs]
        jobs, launches, cells, nbytes = runs[0][1]
        emit(f"{'vc_poa_run_align, ' + name:40s} " + "  ".join(f"{r[0]:.3f}" for r in runs) + " s; the stage (call - median plain call) " +
             "  ".join(f"{t:.3f}" for t in stage) + f" s = " + "  ".join(f"{cells / t / 1e9:.1f}" for t in stage) +
             f" GCUPS ({jobs} jobs, {launches} launches, {cells / 1e9:.2f} G cells, {nbytes / 1e6:.1f} MB copied out)")
    large.release()
    cmd = [sys.executable, os.path.abspath(__file__), "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
    # the shared row body is a template over the gap model: every model named by --parent-gaps beside the parent, two alternated
    # processes each (a warm-up call, then three timed ones)
    for gaps in (a.parent_gaps.split(",") if a.parent_lib else ()):
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + ["--child", "0", "--align", "--gaps", gaps] +
                               (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            emit(f"{'consensus only, ' + gaps + ', ' + ('parent commit' if which == 'parent' else 'this library'):40s} " +
                 "  ".join(f"{a.groups / x:7.1f}" for x in t) + f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
        emit(f"consensus only, {gaps} gaps, {a.depth} members: the parent's {par[0]:.3f} .. {par[-1]:.3f} s (median {med(par):.3f}), this "
             f"library's {cur[0]:.3f} .. {cur[-1]:.3f} s (median {med(cur):.3f}): median against median {(med(cur) / med(par) - 1) * 100:+.2f} %")
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "align")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd +
                           ["--child", "1", "--align", "--queries-per-group", str(a.queries_per_group)], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        info = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]
        emit(f"kernels of one traced call with pairs (a fresh process: 64 groups first, then all), {tot / 1e3:.2f} s: " +
             ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.1f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
        fwd, qfwd = sum(v for k, v in ms.items() if k.startswith("k_lg_fwd")), sum(v for k, v in ms.items() if k.startswith("k_lg_qfwd"))
        if fwd and qfwd:
            emit(f"cells per forward-kernel second: the build's k_lg_fwd {info['build_cells'] / fwd / 1e6:.1f} G/s, the query stage's k_lg_qfwd "
                 f"{info['cells'] / qfwd / 1e6:.1f} G/s (both over the traced process: the 64-group call's cells are not in the numerators)")
    print("wrote", out)
    return 0


def timed_correct(batch, rounds, correct=True, lib=None):
    """-> (seconds, (jobs, launches, cells, bytes) of the `correct` line, (alignments, cells) of the `done` line) of one
    vc_poa_run_correct (global, 5/-4/-8 linear, 0.22 / 0.19 / rounds) on the batch, or with correct=False of the consensus-only
    vc_poa_run_gaps (lib: another library's handle, see parent_handle)"""
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    import re
    import tempfile
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            status = (poa.run_batch_correct(batch, p, capi.VcPoaPruneParams(0.22, 0.19, rounds)) if correct else poa.run_batch(batch, p, lib))[1]
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if int((status != 0).sum()):
        raise RuntimeError(f"{int((status != 0).sum())} groups not computed")
    m = re.search(r"vc_large: correct jobs=(\d+) launches=(\d+) cells=(\d+) bytes=(\d+)", err)
    d = re.search(r"vc_large: done alignments=(\d+) cells=(\d+)", err)
    return dt, tuple(map(int, m.groups())) if m else (0, 0, 0, 0), tuple(map(int, d.groups())) if d else (0, 0)


def main_correct(a):
    """profiles/poa_correct_rate.txt: three plain and three correction calls in one process; with --parent-lib the consensus-only rate
    of this library beside the parent commit's in alternating processes; one kernel trace of the correction call"""
    batch = synth_groups(a)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_correct_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    emit(f"POA groups with haplotype-aware correction: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like errors, "
         f"frac_partial=0, FASTQ), {int(batch.seq_off[-1])} bases; 5/-4/-8, global (kNW); 0.22 / 0.19 / {a.prune_rounds} rounds; one MI355X; "
         f"synchronous; host clock around one call; one untimed call on all groups first, then three calls of each kind in the same process")
    timed_correct(batch, a.prune_rounds, correct=False)
    plain = [timed_correct(batch, a.prune_rounds, correct=False) for _ in range(3)]
    emit(f"{'consensus only (vc_poa_run_gaps)':44s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in plain) +
         f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in plain)} s; {plain[0][2][0]} forward passes, {plain[0][2][1] / 1e9:.1f} G cells)")
    runs = [timed_correct(batch, a.prune_rounds) for _ in range(3)]
    jobs, launches, cells, nbytes = runs[0][1]
    emit(f"{'correction (vc_poa_run_correct, Python copies incl.)':44s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) +
         f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in runs)} s; build and rounds {runs[0][2][0]} forward passes, {runs[0][2][1] / 1e9:.1f} G cells; "
         f"final stage {jobs} jobs in {launches} launches, {cells / 1e9:.1f} G cells, {nbytes / 1e6:.1f} MB copied out of the device)")
    large.release()
    if a.parent_lib:
        # the two libraries alternate, each run a process of its own (a warm-up call, then three timed ones): parent, this, parent, this
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "0", "--correct", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            name = "library of the parent commit" if which == "parent" else "this library"
            emit(f"{'consensus only, ' + name:44s} " + "  ".join(f"{a.groups / x:7.1f}" for x in t) +
                 f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2      # noqa: E731
        emit(f"consensus-only time over the two alternated processes each: the parent's {par[0]:.3f} .. {par[-1]:.3f} s (median {med(par):.3f}), "
             f"this library's {cur[0]:.3f} .. {cur[-1]:.3f} s (median {med(cur):.3f}): median against median {(med(cur) / med(par) - 1) * 100:+.2f} %; "
             f"this library's median lies {'inside (or below)' if med(cur) <= par[-1] else 'ABOVE'} the range of the parent's own runs")
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "correct")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1", "--correct", "--prune-rounds", str(a.prune_rounds), "--groups", str(a.groups),
               "--len", str(a.len), "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"kernel trace: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        emit(f"kernel times of the correction call, a run of its own under rocprofv3 --kernel-trace --stats (64 groups first, then all): "
             f"{tot / 1e3:.2f} s: " + ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    print("wrote", out)
    return 0


def tiled_groups(a):
    """--spans: a.groups groups of one random backbone of a.locus bases plus, per tile of a.len bases, a.depth reads of the tile
    (4 % substitutions, 1 % deletions, 1 % insertions), in tile order, no qualities -> (capi.Batch, (begin, end) span arrays: the
    reads' true ranges, inclusive; none for the backbone)"""
    import numpy as np
    rng = np.random.default_rng(4100)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    groups, begin, end = [], [], []
    for _ in range(a.groups):
        backbone = acgt[rng.integers(0, 4, a.locus)]
        mem = [backbone.tobytes()]
        begin.append(capi.VC_POA_SPAN_NONE); end.append(capi.VC_POA_SPAN_NONE)
        for b in range(0, a.locus, a.len):
            tile = backbone[b:b + a.len]
            for _ in range(a.depth):
                x = rng.random(tile.size)
                s = np.where(x < 0.04, acgt[rng.integers(0, 4, tile.size)], tile)
                rep = np.where(x > 0.99, 2, np.where(x > 0.98, 0, 1))      # an insertion repeats the base, a deletion drops it
                mem.append(np.repeat(s, rep).tobytes())
                begin.append(b); end.append(b + tile.size - 1)
        groups.append(mem)
    return poa.group_batch(groups), (np.array(begin, np.uint32), np.array(end, np.uint32))


def timed_spans(batch, spans=None):
    """-> (seconds, (members, sub_rows, full_rows) of the `spans` line or None, (alignments, cells) of the `done` line, consensus) of
    one vc_poa_run_spans (global, 5/-4/-8 linear) on the batch, or with spans=None of the plain vc_poa_run_gaps on the same groups"""
    p = capi.VcPoaGapParams(**LINEAR_NW)
    import re
    import tempfile
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            cons, status = poa.run_batch(batch, p, spans=spans)
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    if int((status != 0).sum()):
        raise RuntimeError(f"{int((status != 0).sum())} groups not computed")
    m = re.search(r"vc_large: spans members=(\d+) sub_rows=(\d+) full_rows=(\d+)", err)
    d = re.search(r"vc_large: done alignments=(\d+) cells=(\d+)", err)
    return dt, tuple(map(int, m.groups())) if m else None, tuple(map(int, d.groups())) if d else (0, 0), cons


def main_spans(a):
    """profiles/poa_spans_rate.txt: three plain and three span calls on the tiled groups in one process; with --parent-lib the
    consensus-only rate of this library beside the parent commit's on the standard groups, in alternating processes; one kernel
    trace of the span call"""
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_spans_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    batch, spans = tiled_groups(a)
    reads = a.depth * ((a.locus + a.len - 1) // a.len)
    emit(f"POA groups with span-limited alignment: {a.groups} groups of one backbone of {a.locus} bp plus {reads} reads of {a.len} bp tiled over it "
         f"({a.depth} per tile; 4 % substitutions, 1 % deletions, 1 % insertions; no qualities), {int(batch.seq_off[-1])} bases; spans: the reads' "
         f"true ranges; 5/-4/-8, global (kNW); one MI355X; synchronous; host clock around one call; one untimed call of each kind first, then "
         f"three calls of each kind in the same process")
    emit(f"expected before the run: forward cells fall by about len / locus = {a.len / a.locus:.3f}; k_lg_apply and the serial subgraph() in "
         f"k_lg_prep do not fall, so the call's time falls by less")
    timed_spans(batch, spans)
    runs = [timed_spans(batch, spans) for _ in range(3)]
    m, sub_rows, full_rows = runs[0][1]
    emit(f"{'spans (vc_poa_run_spans)':44s} " + "  ".join(f"{a.groups / r[0]:7.2f}" for r in runs) +
         f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in runs)} s; {runs[0][2][0]} forward passes, {runs[0][2][1] / 1e9:.1f} G cells; "
         f"spans line: members={m} sub_rows={sub_rows} full_rows={full_rows}, sub_rows / full_rows = {sub_rows / full_rows:.4f})")
    timed_spans(batch)
    plain = [timed_spans(batch) for _ in range(3)]
    emit(f"{'plain, same groups (vc_poa_run_gaps)':44s} " + "  ".join(f"{a.groups / r[0]:7.2f}" for r in plain) +
         f" groups/s  ({'  '.join(f'{r[0]:.2f}' for r in plain)} s; {plain[0][2][0]} forward passes, {plain[0][2][1] / 1e9:.1f} G cells)")
    med = lambda v: sorted(v)[len(v) // 2]                                # noqa: E731
    same = sum(1 for x, y in zip(runs[0][3], plain[0][3]) if x == y)
    emit(f"span call / plain call: time {med([r[0] for r in runs]) / med([r[0] for r in plain]):.3f} (medians), forward cells "
         f"{runs[0][2][1] / plain[0][2][1]:.3f}; the two consensus sequences are equal in {same} of {a.groups} groups (they are different "
         f"alignments: a plain global alignment stretches a tile's read over the whole locus)")
    large.release()
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "spans")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1", "--spans", "--groups", str(a.groups), "--locus", str(a.locus),
               "--len", str(a.len), "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"kernel trace: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        emit(f"kernel times of one span call, a run of its own under rocprofv3 --kernel-trace --stats: {tot / 1e3:.2f} s: " +
             ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    if a.parent_lib:
        # the plain path on the standard groups; the two libraries alternate, each run a process of its own (a warm-up call, then three
        # timed ones): parent, this, parent, this
        std = 4096
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "0", "--graph", "--groups", str(std), "--len", "1000", "--depth", "32"]
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            name = "library of the parent commit" if which == "parent" else "this library"
            emit(f"{'plain path, ' + name:44s} " + "  ".join(f"{std / x:7.1f}" for x in t) +
                 f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; consensus only, {std} groups of 32 x 1000 bp, a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med2 = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2     # noqa: E731
        emit(f"plain path over the two alternated processes each: the parent's {std / par[-1]:.1f} .. {std / par[0]:.1f} groups/s, this library's "
             f"{std / cur[-1]:.1f} .. {std / cur[0]:.1f}; median against median {(med2(cur) / med2(par) - 1) * 100:+.2f} % in time; the parent's "
             f"documented spread is 408-417 groups/s (profiles/poa_rate.txt)")
    print("wrote", out)
    return 0


def timed_weighted(batch, weights=None, profile=False, msa=False):
    """-> (seconds, bytes the call copied to the host beside consensus and status, consensus) of one global 5/-4/-8 linear call:
    vc_poa_run_gaps, or vc_poa_run_weighted with weights (mode, seq_weight, base_weight) and / or the profile, or vc_poa_run_msa"""
    p = capi.VcPoaGapParams(**LINEAR_NW)
    t0 = time.perf_counter()
    x = poa._run(batch, p, msa_flags=capi.VC_POA_MSA if msa else None, weights=weights, profile=profile)
    dt = time.perf_counter() - t0
    if int((x.status != 0).sum()):
        raise RuntimeError(f"{int((x.status != 0).sum())} groups not computed")
    nbytes = sum(pr.counts.nbytes + len(pr.codes) for pr in x.profiles) if profile else sum(len(r) for m in x.msas for r in m.rows) if msa else 0
    return dt, nbytes, x.cons


def all_mode2(batch, seed=7):
    """every member of the batch with a weight per base, 0..60 -> the arrays of vc_poa_weight_in"""
    import numpy as np
    n, nb = int(batch.win_seq_off[-1]), int(batch.seq_off[-1])
    return np.full(n, 2, np.uint8), np.zeros(n, np.uint32), np.random.default_rng(seed).integers(0, 61, nb, dtype=np.uint32)


def main_weights(a):
    """profiles/poa_weights_rate.txt: (i) the plain path beside the parent commit's library in alternating processes, (ii) every
    member weighted per base beside the plain call, (iii) the profile call beside the consensus-only and the MSA call with the
    bytes each copies out, (iv) the kernel shares of a traced profile call"""
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_weights_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]                                # noqa: E731
    emit(f"POA groups with explicit weights and the consensus profile: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like "
         f"errors, frac_partial=0, FASTQ); 5/-4/-8, global (kNW); one MI355X; synchronous; host clock around one call")
    emit("expected before the run: (i) the plain call launches k_lg_apply<false>, whose weight_of is the body it had, so it stays inside the "
         "parent's own spread; (ii) a per-base weight is one more dependent load per base in k_lg_apply, a lane-serial kernel bound by its "
         "pointer chases: a few per cent at most; (iii) the profile costs k_lg_msa<0> plus one scatter per group and copies (codes + 1) x 4 "
         "bytes per consensus base instead of members bytes per column")
    ok = True
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "0", "--graph", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            name = "library of the parent commit" if which == "parent" else "this library"
            emit(f"(i) {'plain path, ' + name:42s} " + "  ".join(f"{a.groups / x:7.1f}" for x in t) +
                 f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; consensus only, a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med2 = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2     # noqa: E731
        slower, spread = med2(cur) - med2(par), par[-1] - par[0]
        ok = slower <= spread
        emit(f"(i) medians: parent {med2(par):.3f} s, this {med2(cur):.3f} s, difference {slower:+.3f} s ({slower / med2(par) * 100:+.2f} %); the "
             f"parent's own runs of this session spread over {spread:.3f} s ({par[0]:.3f} .. {par[-1]:.3f}): "
             f"{'inside the spread' if ok else 'OUTSIDE the spread'}")
    batch = synth_groups(a)
    timed_weighted(batch)
    plain = [timed_weighted(batch) for _ in range(3)]
    wts = all_mode2(batch)
    weighted = [timed_weighted(batch, weights=wts) for _ in range(3)]
    prof = [timed_weighted(batch, profile=True) for _ in range(3)]
    msa = [timed_weighted(batch, msa=True) for _ in range(3)]
    row = lambda name, runs: emit(f"{name:46s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) +      # noqa: E731
                                  f" groups/s  ({'  '.join(f'{r[0]:.3f}' for r in runs)} s; {runs[0][1]} bytes copied out beside the consensus)")
    row("plain (vc_poa_run_gaps)", plain)
    row("(ii) every member mode 2 (vc_poa_run_weighted)", weighted)
    row("(iii) profile only (vc_poa_run_weighted)", prof)
    row("(iii) alignment rows (vc_poa_run_msa)", msa)
    m = med([r[0] for r in plain])
    emit(f"(ii) weighted / plain {med([r[0] for r in weighted]) / m:.3f}; (iii) profile / plain {med([r[0] for r in prof]) / m:.3f}, rows / plain "
         f"{med([r[0] for r in msa]) / m:.3f} (medians); bytes: profile {prof[0][1]}, rows {msa[0][1]} ({msa[0][1] / max(prof[0][1], 1):.2f}x); the profile "
         f"call's consensus equals the plain call's in {sum(1 for x, y in zip(prof[0][2], plain[0][2]) if x == y)} of {a.groups} groups")
    large.release()
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "weights")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1", "--weights", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"kernel trace: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        emit(f"(iv) kernel times of one weighted call with the profile, a run of its own under rocprofv3 --kernel-trace --stats: {tot / 1e3:.2f} s: " +
             ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    print("wrote", out)
    return 0 if ok else 1


def haplo_groups(a, seed=4100, rate=0.08, snp_every=100):
    """a.groups groups of a.depth reads of about a.len bases -> (capi.Batch, haplotypes per group): a random template per group;
    every second group has a second haplotype with a SNP every snp_every bases, which the odd members are drawn from; every read
    carries `rate` errors, a third each substitutions, deletions and insertions.  numpy only: one pass per group"""
    import numpy as np
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    groups, truth = [], []
    for w in range(a.groups):
        h0 = acgt[rng.integers(0, 4, a.len)]
        h1 = h0.copy()
        two = w % 2 == 1
        if two:
            pos = np.arange(snp_every // 2, a.len, snp_every)
            h1[pos] = acgt[(np.searchsorted(acgt, h0[pos]) + rng.integers(1, 4, pos.size)) % 4]
        reads = []
        for k in range(a.depth):
            src = h1 if two and k % 2 else h0
            u = rng.random(a.len)
            r = np.where((u >= rate / 3) & (u < 2 * rate / 3), acgt[rng.integers(0, 4, a.len)], src)
            ins = (u >= 2 * rate / 3) & (u < rate)
            keep = u >= rate / 3
            r, ins = r[keep], ins[keep]
            out = np.repeat(r, 1 + ins)
            at = np.cumsum(1 + ins)[ins] - 1                             # the copy behind every base with an insertion
            out[at] = acgt[rng.integers(0, 4, at.size)]
            reads.append(out.tobytes())
        groups.append(reads)
        truth.append(2 if two else 1)
    return poa.group_batch(groups), truth


def timed_haplotypes(batch, hap=None):
    """-> (seconds, bytes copied out beside consensus and status, consensus, haplotypes per group) of one global 5/-4/-8 linear call
    of vc_poa_run_haplotypes with the rule's defaults"""
    p = capi.VcPoaGapParams(**LINEAR_NW)
    t0 = time.perf_counter()
    cons, status, res, raw = poa.run_batch_haplotypes(batch, p, hap or poa.hap_params())
    dt = time.perf_counter() - t0
    if int((status != 0).sum()):
        raise RuntimeError(f"{int((status != 0).sum())} groups not computed")
    return dt, raw["bytes"], cons, [len(h.sizes) for h in res]


def main_haplotypes(a):
    """profiles/poa_haplo_rate.txt: (i) the plain path beside the parent commit's library in alternating processes, (ii) the
    haplotype call beside the plain call and the graph call in one process with the bytes each copies out, (iii) the kernel
    shares of a traced haplotype call"""
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_haplo_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]                                # noqa: E731
    emit(f"POA groups split into haplotypes: {a.groups} groups of {a.depth} x {a.len} bp, every second one from two haplotypes (a SNP every "
         f"100 bases, half of the reads each), 8 % read errors, FASTA, numpy seed 4100; 5/-4/-8, global (kNW), the rule's defaults; one MI355X; "
         f"synchronous; host clock around one call")
    emit("expected before the run: (i) the plain call launches no new kernel and heaviest_bundle's whole-graph view folds to the code it "
         "had, so it stays inside the parent's own spread; (ii) the haplotype call adds k_lg_graph<0>, k_lg_hap and k_lg_hapcons behind a "
         "build that k_lg_apply and k_lg_fwd dominate: k_lg_hap's serial loops over members per column and k_lg_hapcons's lane-serial "
         "bundle (one more bundle per haplotype) should stay a few per cent of the call, and it copies far fewer bytes than the graph "
         "call; nothing is asserted about the stage's own speed")
    ok = True
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "0", "--graph", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"{which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1                          # nothing more is started on the device after a failed run
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            name = "library of the parent commit" if which == "parent" else "this library"
            emit(f"(i) {'plain path, ' + name:42s} " + "  ".join(f"{a.groups / x:7.1f}" for x in t) +
                 f" groups/s  ({'  '.join(f'{x:.3f}' for x in t)} s; consensus only on the standard vc_synth groups, a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med2 = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2     # noqa: E731
        slower, spread = med2(cur) - med2(par), par[-1] - par[0]
        ok = slower <= spread
        emit(f"(i) medians: parent {med2(par):.3f} s, this {med2(cur):.3f} s, difference {slower:+.3f} s ({slower / med2(par) * 100:+.2f} %); the "
             f"parent's own runs of this session spread over {spread:.3f} s ({par[0]:.3f} .. {par[-1]:.3f}): "
             f"{'inside the spread' if ok else 'OUTSIDE the spread'}")
    else:
        emit("(i) not run: no --parent-lib was given")
    batch, truth = haplo_groups(a)
    timed_graph(batch, graph=False)
    plain = [timed_graph(batch, graph=False)[:2] for _ in range(3)]
    haps = [timed_haplotypes(batch) for _ in range(3)]
    graph = [timed_graph(batch, 0)[:2] for _ in range(3)]
    row = lambda name, runs: emit(f"{name:46s} " + "  ".join(f"{a.groups / r[0]:7.1f}" for r in runs) +      # noqa: E731
                                  f" groups/s  ({'  '.join(f'{r[0]:.3f}' for r in runs)} s; {runs[0][1]} bytes copied out beside the consensus)")
    row("plain (vc_poa_run_gaps)", plain)
    row("(ii) haplotypes (vc_poa_run_haplotypes)", haps)
    row("(ii) graph tables (vc_poa_run_graph)", graph)
    m = med([r[0] for r in plain])
    found = haps[0][3]
    emit(f"(ii) haplotypes / plain {med([r[0] for r in haps]) / m:.3f}, graph / plain {med([r[0] for r in graph]) / m:.3f} (medians); groups with the "
         f"planted number of haplotypes: {sum(1 for x, y in zip(found, truth) if x == y)} of {a.groups} "
         f"({sum(1 for x in truth if x == 2)} planted with two)")
    large.release()
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "haplotypes")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1", "--haplotypes", "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"kernel trace: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        emit(f"(iii) kernel times of one haplotype call, a run of its own under rocprofv3 --kernel-trace --stats: {tot / 1e3:.2f} s: " +
             ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    else:
        emit("(iii) not run: --no-trace")
    print("wrote", out)
    return 0 if ok else 1


LINEAR_NW = dict(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)


def resume_call(batch, start=None, qbatch=None, outputs=True, entry="vc_poa_run_from"):
    """One library call with only the call on the clock -> (seconds, consensus per group, VC_LARGE_LOG lines, pairs digest or None).
    entry vc_poa_run_from: from = the packed `start` (a list of resumable PoaGraph, or None: from nothing), the graph tables and
    the state as outputs when `outputs`, the queries of qbatch with their pairs; entry vc_poa_run_align: the same groups and
    queries through the entry that builds them again."""
    import ctypes as C
    import hashlib
    import tempfile
    lib = capi.load_hip()
    p = capi.VcPoaGapParams(**LINEAR_NW)
    gin, keep = poa._graph_in(start) if start is not None else (None, None)
    cons, off, status, r, vb = poa._result_buffers(batch, sum(g.n_nodes for g in start) if start is not None else 0)
    g, st = (capi.VcPoaGraphOut(), capi.VcPoaStateOut()) if outputs else (None, None)
    qv = al = None
    if qbatch is not None:
        qv = qbatch.as_struct()
        qv.seq_begin = qv.seq_end = qv.win_fasta = qv.seq_has_qual = qv.quals = None
        al = capi.VcPoaAlignOut(flags=capi.VC_POA_ALIGN_PAIRS)
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            if entry == "vc_poa_run_from":
                rc = lib.vc_poa_run_from(C.byref(p), ref(gin), C.byref(vb), C.byref(r), None, None, ref(g), ref(st), ref(qv), ref(al))
            else:
                rc = lib.vc_poa_run_align(C.byref(p), C.byref(vb), C.byref(r), None, None, ref(qv), ref(al))
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        err = log.read().decode()
    del keep
    if rc != 0 or int((status[:batch.n_windows] != 0).sum()):
        raise RuntimeError(f"{entry} failed ({rc}): {lib.vc_poa_last_error().decode()}; groups not computed: {int((status != 0).sum())}")
    digest = None
    if al is not None:
        nq = int(al.n_queries)
        po = poa._table(al.pair_off, nq + 1)
        h = hashlib.sha256(poa._table(al.score, nq).tobytes() + po.tobytes())
        h.update(poa._table(al.pair_node, int(po[-1])).tobytes() + poa._table(al.pair_pos, int(po[-1])).tobytes())
        digest = h.hexdigest()
    n = batch.n_windows
    return dt, [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)], err, digest


def resume_batches(a, batch):
    """-> (all members per group, the first 3/4, the last 1/4, no member, one query per group: a member with 5 % substitutions)"""
    import random
    rng = random.Random(4102)
    groups, queries = [], []
    for w in range(batch.n_windows):
        seqs, quals, _, _ = batch.window(w)
        groups.append(list(zip(seqs, quals)))
        s = bytearray(rng.choice(seqs))
        for _ in range(max(1, len(s) // 20)):
            s[rng.randrange(len(s))] = rng.choice(b"ACGT")
        queries.append([bytes(s)])
    k = a.depth - max(1, a.depth // 4)
    gb = poa.group_batch
    return gb(groups), gb([g[:k] for g in groups]), gb([g[k:] for g in groups]), gb([[] for _ in groups]), poa.query_batch(queries), k


def stored_graphs(batch):
    """the groups of the batch built from nothing with their state -> list of resumable PoaGraph"""
    x = poa._run(batch, capi.VcPoaGapParams(**LINEAR_NW), graph=True, state=True)
    if int((x.status != 0).sum()):
        raise RuntimeError("groups not computed")
    return x.graphs


def main_resume(a):
    """profiles/poa_resume_rate.txt: (a) queries against stored graphs beside vc_poa_run_align, (b) adding a quarter of the members
    beside the one-shot build, (c) k_lg_load beside k_lg_apply in a traced run of its own, (d) the plain path beside the parent"""
    import re
    whole, head, tail, none, qb, k = resume_batches(a, synth_groups(a))
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_resume_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    ok = True
    fmt = lambda ts: "  ".join(f"{t:.3f}" for t in ts)  # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    emit(f"POA groups that go on from a stored graph: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like errors, "
         f"frac_partial=0, FASTQ); 5/-4/-8, global (kNW); one MI355X; synchronous; host clock around the library call alone (the stored "
         f"graphs are packed before it, nothing is copied out inside it); one process, one untimed call of each kind first, then three")
    # (a)
    graphs = stored_graphs(whole)
    load = lambda err: (re.search(r"vc_large: load .*", err) or [""])[0]  # noqa: E731
    emit(f"(a) expectation: a query call on stored graphs costs the load plus the query stage, a small fraction (below a quarter) of the "
         f"call that builds the groups again, because it skips the {a.depth} dependent steps of the build")
    resume_call(none, graphs, qb, outputs=False)
    fr = [resume_call(none, graphs, qb, outputs=False) for _ in range(3)]
    resume_call(whole, None, qb, outputs=False, entry="vc_poa_run_align")
    al = [resume_call(whole, None, qb, outputs=False, entry="vc_poa_run_align") for _ in range(3)]
    same = fr[0][1] == al[0][1] and fr[0][3] == al[0][3]
    done = re.search(r"vc_large: done .*", fr[0][2])[0]
    emit(f"    vc_poa_run_from, stored graphs of {a.depth} members, no new member, 1 query per group   {fmt(r[0] for r in fr)} s   [{load(fr[0][2])}; {done}]")
    emit(f"    vc_poa_run_align, the same groups built again, the same queries                     {fmt(r[0] for r in al)} s")
    ratio = med([r[0] for r in fr]) / med([r[0] for r in al])
    met = ratio < 0.25
    emit(f"    median against median {ratio:.4f} of the rebuild ({1 / ratio:.1f}x): expectation {'met' if met else 'NOT met'}; consensus, scores "
         f"and pairs of the two {'identical' if same else 'DIFFERENT'}")
    ok = ok and met and same
    del graphs
    # (b)
    emit(f"(b) expectation: adding the last {a.depth - k} of {a.depth} members to stored graphs costs about {a.depth - k}/{a.depth} of the "
         f"one-shot build plus the load; checked as below half of it (the last members meet the largest graphs)")
    graphs = stored_graphs(head)
    resume_call(tail, graphs)
    ex = [resume_call(tail, graphs) for _ in range(3)]
    del graphs
    resume_call(whole)
    one = [resume_call(whole) for _ in range(3)]
    same = ex[0][1] == one[0][1]
    emit(f"    vc_poa_run_from, stored graphs of {k} members + {a.depth - k} new, graph tables and state out   {fmt(r[0] for r in ex)} s   [{load(ex[0][2])}]")
    emit(f"    vc_poa_run_from from nothing, {a.depth} members, graph tables and state out                {fmt(r[0] for r in one)} s")
    ratio = med([r[0] for r in ex]) / med([r[0] for r in one])
    met = ratio < 0.5
    emit(f"    median against median {ratio:.4f} of the one-shot build ({(a.depth - k) / a.depth:.4f} would be the members' share): expectation "
         f"{'met' if met else 'NOT met'}; consensus of the two {'identical' if same else 'DIFFERENT'}")
    ok = ok and met and same
    large.release()
    cmd = [sys.executable, os.path.abspath(__file__), "--groups", str(a.groups), "--len", str(a.len), "--depth", str(a.depth), "--resume"]
    # (c)
    if not a.no_trace:
        d = os.path.join(a.trace_dir, "resume")
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + cmd + ["--child", "1"],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"(c) rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1                              # nothing more is started on the device after a failed run
        ms = kernel_shares(d)
        tot = sum(ms.values())
        ld, ap = sum(v for n, v in ms.items() if n.startswith("k_lg_load")), sum(v for n, v in ms.items() if n.startswith("k_lg_apply"))
        emit(f"(c) kernels of a traced process of its own (build {k} members with the state, then add {a.depth - k}), {tot / 1e3:.2f} s: k_lg_load "
             f"{ld:.1f} ms beside k_lg_apply {ap:.1f} ms ({ld / max(ap, 1e-9) * 100:.2f} % of it); all: " +
             ", ".join(f"{n} {v:.1f} ms" for n, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    # (d)
    if a.parent_lib:
        secs = {"parent": [], "this": []}
        for which in ("parent", "this", "parent", "this"):
            p = subprocess.run(cmd + ["--child", "0"] + (["--parent-lib", os.path.abspath(a.parent_lib)] if which == "parent" else []),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"(d) {which} library: run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                return 1
            t = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            secs[which] += t
            emit(f"(d) {'consensus only, ' + ('parent commit' if which == 'parent' else 'this library'):32s} " +
                 "  ".join(f"{a.groups / x:7.1f}" for x in t) + f" groups/s  ({fmt(t)} s; a process of its own)")
        par, cur = sorted(secs["parent"]), sorted(secs["this"])
        med2 = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
        emit(f"(d) consensus only over the two alternated processes each: the parent's {par[0]:.3f} .. {par[-1]:.3f} s (median {med2(par):.3f}), "
             f"this library's {cur[0]:.3f} .. {cur[-1]:.3f} s (median {med2(cur):.3f}): median against median {(med2(cur) / med2(par) - 1) * 100:+.2f} %; "
             f"the parent's documented spread is 408-417 groups/s, about 2 %")
    print("wrote", out)
    return 0 if ok else 1


def assign_inputs(a):
    """the groups, and --queries queries: members of the groups in turn, mutated (4 % substitutions, 1 % deletions, 1 % insertions)"""
    import random
    batch = synth_groups(a)
    rng = random.Random(4200)
    wso, so = batch.win_seq_off, batch.seq_off
    queries = []
    for k in range(a.queries):
        w = k % batch.n_windows
        s = int(wso[w]) + rng.randrange(int(wso[w + 1]) - int(wso[w]))
        out = bytearray()
        for ch in batch.bases[int(so[s]):int(so[s + 1])].tobytes():
            x = rng.random()
            if x < 0.01:
                continue
            out.append(rng.choice(b"ACGT") if x < 0.05 else ch)
            if x > 0.99:
                out.append(rng.choice(b"ACGT"))
        queries.append(bytes(out))
    return batch, queries


def _logged(f):
    """f() with VC_LARGE_LOG=1 -> (seconds, f's result, the library's stderr lines)"""
    import tempfile
    with tempfile.TemporaryFile() as log:
        saved = os.dup(2)
        os.dup2(log.fileno(), 2)
        os.environ["VC_LARGE_LOG"] = "1"
        try:
            t0 = time.perf_counter()
            res = f()
            dt = time.perf_counter() - t0
        finally:
            del os.environ["VC_LARGE_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
        log.seek(0)
        return dt, res, log.read().decode()


def _kv(err, what):
    line = [l for l in err.splitlines() if l.startswith("vc_large: " + what)][-1]
    return {k: int(v) for k, v in (t.split("=") for t in line.split()[2:])}


def assign_routes(a, batch, queries):
    """-> (plain(), assign(), align()): the build alone, the assign call, and the existing route to the same table --
    vc_poa_run_align without pairs on the queries repeated per group -- each -> (seconds, result, log)"""
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    qb = poa.query_batch([queries])
    rep = poa.query_batch([queries] * batch.n_windows)
    return (lambda: _logged(lambda: poa.run_batch(batch, p)),
            lambda: _logged(lambda: poa.run_batch_assign(batch, qb, p, capi.VC_POA_ASSIGN_SCORES)),
            lambda: _logged(lambda: poa.run_batch_align(batch, rep, p, 0)))


def main_assign(a):
    """profiles/poa_assign_rate.txt: the assign call beside the existing route to the same scores, both in one process on the same
    pairs; one kernel trace of a quarter of the pairs through both"""
    out = a.out if a.out != os.path.join(ROOT, "profiles", "poa_rate.txt") else os.path.join(ROOT, "profiles", "poa_assign_rate.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        open(out, "w").write("\n".join(lines) + "\n")
    batch, queries = assign_inputs(a)
    pairs = a.groups * a.queries
    emit(f"Queries assigned to POA groups: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100), {a.queries} queries (mutated members, "
         f"about {a.len} bp), {pairs} pairs; 5/-4/-8, global (kNW), one strand; one MI355X; synchronous; host clock around one call, the "
         f"build included; both routes in one process, one untimed call of each first, then alternating")
    emit("expected before the run: the cells computed are equal; the int32 cells stored fall by about rows / n_slots (ring_cells / full_cells "
         "below); the launches fall to a handful; so the assign call should be faster than vc_poa_run_align without pairs on the queries "
         "repeated per group")
    plain, assign, align = assign_routes(a, batch, queries)
    plain(); assign(); align()
    tp = [plain()[0] for _ in range(2)]
    runs_s, runs_q = [], []
    for _ in range(2):
        runs_s.append(assign())
        runs_q.append(align())
    ks, kq = _kv(runs_s[0][2], "assign"), _kv(runs_q[0][2], "align")
    table = runs_s[0][1][3]
    old = runs_q[0][1][2]
    same = all(int(table[k, w]) == old[w][k].score for w in range(a.groups) for k in range(0, a.queries, max(1, a.queries // 64)))
    build = min(tp)
    cells = kq["cells"]
    for name, runs, launches in (("assign (vc_poa_run_assign, scores table)", runs_s, ks["launches"]), ("existing route (vc_poa_run_align, no pairs)", runs_q, kq["launches"])):
        t = [r[0] for r in runs]
        emit(f"{name:46s} " + "  ".join(f"{x:7.3f}" for x in t) + " s per call; stage = call - build: " +
             "  ".join(f"{pairs / max(x - build, 1e-9):9.0f}" for x in t) + " pairs/s, " +
             "  ".join(f"{cells / max(x - build, 1e-9) / 1e9:6.2f}" for x in t) + f" GCUPS; {launches} forward launches")
    emit(f"build alone (vc_poa_run_gaps): {'  '.join(f'{x:.3f}' for x in tp)} s; forward cells of the pairs (rows x columns): {cells / 1e9:.2f} G")
    emit(f"assign line: slots_max={ks['slots_max']} ring_cells={ks['ring_cells']} full_cells={ks['full_cells']}, ring_cells / full_cells = "
         f"{ks['ring_cells'] / max(ks['full_cells'], 1):.5f}; sampled scores equal between the routes: {same}")
    ts, tq = sorted(r[0] for r in runs_s), sorted(r[0] for r in runs_q)
    spread = tq[-1] - tq[0]
    ok = same and (ts[0] + ts[-1]) / 2 <= (tq[0] + tq[-1]) / 2 + spread
    emit(f"bar: the assign call's mean {(ts[0] + ts[-1]) / 2:.3f} s against the existing route's {(tq[0] + tq[-1]) / 2:.3f} s + its spread between "
         f"two runs {spread:.3f} s: {'met' if ok else 'MISSED'} (call time ratio {(ts[0] + ts[-1]) / (tq[0] + tq[-1]):.3f})")
    large.release()
    if ok and not a.no_trace:
        d = os.path.join(a.trace_dir, "assign")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--child", "1", "--assign", "--groups", str(max(a.groups // 2, 1)),
               "--queries", str(max(a.queries // 2, 1)), "--len", str(a.len), "--depth", str(a.depth)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            emit(f"kernel trace: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
            return 1
        ms = kernel_shares(d)
        tot = sum(ms.values())
        emit(f"kernel times of one assign call and one call of the existing route on a quarter of the pairs, a run of its own under rocprofv3 "
             f"--kernel-trace --stats: {tot / 1e3:.2f} s: " +
             ", ".join(f"{k} {v:.1f} ms ({v / tot * 100:.2f} %)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1])))
    print("wrote", out)
    return 0 if ok else 1


def child(a):
    """one algorithm's call, for the kernel trace: warm-up and timed call as above, JSON on stdout"""
    if a.assign:                                  # the traced run: one assign call and one call of the existing route
        batch, queries = assign_inputs(a)
        _, assign, align = assign_routes(a, batch, queries)
        print(json.dumps(dict(assign=assign()[0], align=align()[0])))
        return
    if a.resume and a.child == 1:                 # the traced run: build 3/4 of the members with the state, then add the rest
        _, head, tail, _, _, _ = resume_batches(a, synth_groups(a))
        small = min(64, head.n_windows)
        resume_call(tail.slice(0, small), stored_graphs(head.slice(0, small)))
        dt = resume_call(tail, stored_graphs(head))[0]
        print(json.dumps(dict(seconds=dt)))
        return
    if a.haplotypes:                              # the traced run: one haplotype call
        dt, nbytes, _, found = timed_haplotypes(haplo_groups(a)[0])
        print(json.dumps(dict(seconds=dt, bytes=nbytes, two=sum(1 for x in found if x == 2))))
        return
    if a.weights:                                 # the traced run: one call with every member weighted per base and the profile
        batch = synth_groups(a)
        dt, nbytes, _ = timed_weighted(batch, weights=all_mode2(batch), profile=True)
        print(json.dumps(dict(seconds=dt, bytes=nbytes)))
        return
    if a.spans:                                   # the traced run: one span call on the tiled groups
        batch, spans = tiled_groups(a)
        dt, line, done, _ = timed_spans(batch, spans)
        print(json.dumps(dict(seconds=dt, spans=line, cells=done[1])))
        return
    if a.correct:
        batch = synth_groups(a)
        if a.child == 0:                         # consensus only, three calls after a full warm-up (this library's or the parent's)
            lib = parent_handle(a.parent_lib) if a.parent_lib else None
            timed_correct(batch, a.prune_rounds, correct=False, lib=lib)
            print(json.dumps(dict(seconds=[timed_correct(batch, a.prune_rounds, correct=False, lib=lib)[0] for _ in range(3)])))
            return
        timed_correct(batch.slice(0, min(64, batch.n_windows)), a.prune_rounds)
        dt, stage, done = timed_correct(batch, a.prune_rounds)
        print(json.dumps(dict(seconds=dt, jobs=stage[0], cells=stage[2], build_cells=done[1])))
        return
    if (a.align or a.resume) and a.child == 0:    # consensus only (vc_poa_run_gaps, global, --gaps), this library's or the parent's
        batch = synth_groups(a)
        g, e, q, c = GAPS[a.gaps] or (-8, -8, -8, -8)
        p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=g, gap_extend=e, gap_open2=q, gap_extend2=c)
        lib = parent_handle(a.parent_lib) if a.parent_lib else None
        secs = []
        for k in range(4):                        # the first call grows the buffer cache
            t0 = time.perf_counter()
            status = poa.run_batch(batch, p, lib)[1]
            secs.append(time.perf_counter() - t0)
            if int((status != 0).sum()):
                raise RuntimeError("groups not computed")
        print(json.dumps(dict(seconds=secs[1:])))
        return
    if a.align:
        gb, qb = align_batches(a, synth_groups(a))
        small = a.groups if a.groups <= 64 else 64
        timed_align(gb.slice(0, small), qb.slice(0, small), 1)
        dt, (jobs, _, cells, _) = timed_align(gb, qb, 1)
        build_cells = timed(gb, 1, None)[4]                             # the same build once more, for its cells (k_lg_fwd runs twice)
        print(json.dumps(dict(seconds=dt, jobs=jobs, cells=cells, build_cells=2 * build_cells)))
        return
    if a.graph:
        batch = synth_groups(a)
        if a.child == 0:                          # consensus only, three calls after a full warm-up (the parent library's run)
            lib = parent_handle(a.parent_lib) if a.parent_lib else None
            timed_graph(batch, graph=False, lib=lib)
            print(json.dumps(dict(seconds=[timed_graph(batch, graph=False, lib=lib)[0] for _ in range(3)])))
            return
        if a.child == 2:
            os.environ["VC_LARGE_GRAPH_WALK"] = "1"
        timed_graph(batch.slice(0, min(64, batch.n_windows)), 7)
        dt, nbytes, graphs = timed_graph(batch, 7)
        import hashlib
        h = hashlib.sha256()
        for g in graphs:                          # the two routes must write the same paths
            h.update(g.path_off.tobytes() + g.path_node.tobytes())
        print(json.dumps(dict(seconds=dt, bytes=nbytes, paths=h.hexdigest())))
        return
    if a.strand:
        batch = synth_groups(a)
        if a.child:
            batch = flip_members(batch)[0]
        timed_strand(batch.slice(0, min(64, batch.n_windows)), a.gaps, bool(a.child))
        dt, _, _, n_al, cells = timed_strand(batch, a.gaps, bool(a.child))
        print(json.dumps(dict(seconds=dt, alignments=n_al, cells=cells)))
        return
    if a.msa:
        batch = synth_groups(a)
        timed_msa(batch.slice(0, min(64, batch.n_windows)), a.child)
        dt, nbytes, n_al, cells = timed_msa(batch, a.child)
        print(json.dumps(dict(seconds=dt, alignments=n_al, cells=cells, bytes=nbytes)))
        return
    batch = synth_groups(a)
    dt, _, status, n_al, cells = timed(batch, a.child, "small", a.gaps)
    print(json.dumps(dict(seconds=dt, alignments=n_al, cells=cells, ok=int((status == 0).sum()))))


def cpu_reference(batch, idx, alg, threads, kind="sse41"):
    import make_poa
    import oracle_api as oa
    lib = oa.load_ref(kind)

    def one(w):
        seqs, quals, _, _ = batch.window(w)
        return make_poa.ref_consensus(lib, list(zip(seqs, quals)), alg, 5, -4, -8)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        out = list(ex.map(one, idx))
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--len", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--cpu-sample", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poa_rate.txt"))
    ap.add_argument("--trace-dir", default="/tmp/poa_rate_trace")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--gaps", choices=sorted(GAPS), default="linear")
    ap.add_argument("--msa", action="store_true", help="measure vc_poa_run_msa beside the consensus-only call (profiles/poa_msa_rate.txt)")
    ap.add_argument("--strand", action="store_true", help="measure vc_poa_run_strand beside the plain call (profiles/poa_strand_rate.txt)")
    ap.add_argument("--graph", action="store_true", help="measure vc_poa_run_graph beside the consensus-only call (profiles/poa_graph_rate.txt)")
    ap.add_argument("--align", action="store_true", help="measure vc_poa_run_align's query stage beside the plain call (profiles/poa_align_rate.txt)")
    ap.add_argument("--correct", action="store_true", help="measure vc_poa_run_correct beside the consensus-only call (profiles/poa_correct_rate.txt)")
    ap.add_argument("--resume", action="store_true", help="measure vc_poa_run_from: stored-graph queries, extending, k_lg_load (profiles/poa_resume_rate.txt)")
    ap.add_argument("--spans", action="store_true", help="measure vc_poa_run_spans beside the plain call on tiled groups (profiles/poa_spans_rate.txt; "
                                                         "--groups defaults to 512 here)")
    ap.add_argument("--weights", action="store_true", help="measure vc_poa_run_weighted: the plain path beside --parent-lib, weights, the profile "
                                                           "(profiles/poa_weights_rate.txt)")
    ap.add_argument("--assign", action="store_true", help="measure vc_poa_run_assign beside vc_poa_run_align without pairs on the queries repeated "
                                                          "per group (profiles/poa_assign_rate.txt; --groups defaults to 256)")
    ap.add_argument("--haplotypes", action="store_true", help="measure vc_poa_run_haplotypes beside the plain and the graph call on groups half "
                                                              "of which hold two haplotypes (profiles/poa_haplo_rate.txt)")
    ap.add_argument("--queries", type=int, default=1024, help="--assign: queries of the call")
    ap.add_argument("--locus", type=int, default=8000, help="--spans: bases of a group's backbone, tiled by reads of --len bases, --depth per tile")
    ap.add_argument("--prune-rounds", type=int, default=3, help="--correct: num_prune (default 3)")
    ap.add_argument("--queries-per-group", type=int, default=32, help="--align: mutated members per group beside the held-out one")
    ap.add_argument("--parent-gaps", default="linear,affine,convex", help="--align --parent-lib: the gap models compared with the parent's library")
    ap.add_argument("--parent-lib", default=None, help="--graph / --align / --correct: a libvechat_hip.so of the parent commit, for its consensus-only rate")
    ap.add_argument("--check", type=int, default=2, help="--graph: groups whose GFA is compared with the CPU restatement's")
    ap.add_argument("--append", action="store_true", help="--strand: keep what the output file holds and write below it")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.spans and "--groups" not in sys.argv:
        a.groups = 512
    if a.assign and "--groups" not in sys.argv:
        a.groups = 256
    if a.child is not None:
        return child(a)
    if a.assign:
        return main_assign(a)
    if a.haplotypes:
        return main_haplotypes(a)
    if a.weights:
        return main_weights(a)
    if a.spans:
        return main_spans(a)
    if a.resume:
        return main_resume(a)
    if a.correct:
        return main_correct(a)
    if a.align:
        return main_align(a)
    if a.graph:
        return main_graph(a)
    if a.strand:
        return main_strand(a)
    if a.msa:
        return main_msa(a)
    batch = synth_groups(a)
    bases = int(batch.seq_off[-1])
    scores, entry = ("5/-4/-8", "vc_poa_run") if GAPS[a.gaps] is None else \
        (f"5/-4/{'/'.join(map(str, GAPS[a.gaps]))} ({a.gaps} gaps)", "vc_poa_run_gaps")
    lines = [f"POA groups: {a.groups} groups of {a.depth} x {a.len} bp (vc_synth seed 4100, PacBio-like errors, frac_partial=0, FASTQ), "
             f"{bases} bases; scores {scores}; one MI355X; {entry}, synchronous; host clock around one call; before it one untimed call on all groups (the first algorithm: the buffer cache grows) or on 64"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):                               # the file is rewritten after every line: a run cut short keeps what it measured
        lines.append(line)
        print(line, flush=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    emit(lines.pop())
    results = {}
    for alg in (0, 1, 2):
        dt, cons, status, n_al, cells = timed(batch, alg, "full" if alg == 0 else "small", a.gaps)
        results[alg] = dict(seconds=dt, cons=cons, ok=int((status == 0).sum()), alignments=n_al, cells=cells)
        emit(f"{NAMES[alg]:18s} {dt:8.2f} s  {a.groups / dt:8.1f} groups/s  {cells / dt / 1e9:7.2f} GCUPS  "
             f"({n_al} alignments, {cells / 1e9:.2f} G cells, {results[alg]['ok']} of {a.groups} VC_WIN_OK)")
    large.release()
    if a.cpu_sample and GAPS[a.gaps] is not None:
        emit("reference: none -- oracle/_ref builds spoa's engine through Create(type, m, n, g) only (linear gaps)")
    elif a.cpu_sample:
        import random
        idx = sorted(random.Random(1).sample(range(a.groups), min(a.cpu_sample, a.groups)))
        emit(f"reference: spoa (oracle/_ref libvcref_sse41.so, vcref_spoa_consensus) on {len(idx)} of the groups, {a.threads} host threads; "
             f"device consensus compared with it and with the scalar build (libvcref_sisd.so):")
        for alg in (0, 1, 2):
            dt, out = cpu_reference(batch, idx, alg, a.threads)
            _, scalar = cpu_reference(batch, idx, alg, a.threads, "sisd")
            dev = results[alg]["cons"]
            same = sum(1 for w, (rc, c) in zip(idx, out) if rc == 0 and c == dev[w])
            same_s = sum(1 for w, (rc, c) in zip(idx, scalar) if rc == 0 and c == dev[w])
            rate = len(idx) / dt
            emit(f"  {NAMES[alg]:18s} {dt:7.2f} s  {rate:8.1f} groups/s  device / reference {a.groups / results[alg]['seconds'] / rate:.2f}x  "
                 f"consensus equal to the SIMD build in {same}, to the scalar build in {same_s} of {len(idx)}")
    if not a.no_trace:
        emit("kernel time shares, each algorithm's call in a run of its own under rocprofv3 --kernel-trace --stats:")
        for alg in (0, 1, 2):
            d = os.path.join(a.trace_dir, f"alg{alg}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", str(alg), "--groups", str(a.groups), "--len", str(a.len),
                   "--depth", str(a.depth), "--gaps", a.gaps]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                emit(f"  {NAMES[alg]}: rocprofv3 run failed ({p.returncode}): {p.stderr.strip().splitlines()[-1:]}")
                break
            ms = kernel_shares(d)
            tot = sum(ms.values())
            shares = ", ".join(f"{k} {v / tot * 100:.1f} % ({v / 1e3:.2f} s)" for k, v in sorted(ms.items(), key=lambda kv: -kv[1]))
            wall = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][-1]["seconds"]
            emit(f"  {NAMES[alg]:18s} kernels {tot / 1e3:.2f} s of {wall:.2f} s wall (traced; a fresh process, its first call allocates the buffer cache): {shares}")
    print("wrote", a.out)


if __name__ == "__main__":
    sys.exit(main())
