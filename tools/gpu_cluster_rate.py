#!/usr/bin/env python3
"""Rate of the device clusterer (vc_cluster) on simulated reads of a few dozen loci; writes profiles/cluster_rate.txt.

  python tools/gpu_cluster_rate.py [--reads 2000] [--read-len 5000] [--loci 32] [--locus-len 6000] [--err 0.06] [--out profiles/cluster_rate.txt]

The set is the one of tools/gpu_overlap_rate.py (2 000 reads of 5 kb, both strands, 6 % errors per read) drawn from a few dozen
unrelated loci instead of one genome.  Reported: ms per warm vc_cluster call (best of three, host clock around the synchronous
call, uploads and the copy back included), records/s, links, rounds and clusters, the kernel shares from a
`rocprofv3 --kernel-trace --stats` run of its own (a child process, no counters), for the components step (k_cl_init, k_cl_hook,
k_cl_flatten) the time expected from the bytes it moves and the copy bandwidth tools/hbm_bw.hip reports in the same session --
stated before the figure -- and the wall time of the cluster command beside the overlap command on the same reads.  There is no
outside baseline (no clusterer here) and no threshold: the file records what was measured.  Needs the GPU."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_overlap_rate import simulate  # noqa: E402
from gpu_scrub_rate import copy_bandwidth  # noqa: E402


def reads_of(a):
    """the reads locus by locus, then shuffled: (reads, locus per read)"""
    reads, locus = [], []
    for x in range(a.loci):
        mine = simulate(a.reads // a.loci + (x < a.reads % a.loci), a.read_len, a.locus_len, a.err, seed=3 + x)
        reads += mine
        locus += [x] * len(mine)
    order = np.random.default_rng(1).permutation(len(reads))
    return [reads[i] for i in order], [locus[i] for i in order]


def measure(a):
    from vechat_amd import cluster, overlap
    reads, locus = reads_of(a)
    ov = overlap.find_overlaps(reads, None, **overlap.PRESETS["ava-ont"])
    lengths = [len(r) for r in reads]
    times, res = [], None
    for _ in range(4):                                          # the first call is the warm-up
        t0 = time.perf_counter()
        res = cluster.run(lengths, ov)
        times.append(time.perf_counter() - t0)
    return reads, locus, ov, res, min(times[1:])


def kernel_rows(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "cl", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--read-len", str(a.read_len),
               "--loci", str(a.loci), "--locus-len", str(a.locus_len), "--err", str(a.err)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    return [r for r in rows if "k_cl_" in r["Name"]]


def command_times(reads):
    """wall seconds of the overlap command and of the cluster command on one FASTQ, process start-up included"""
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    out = []
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "reads.fastq")
        with open(fq, "w") as f:
            for i, r in enumerate(reads):
                f.write(f"@r{i}\n{r.decode()}\n+\n{'5' * len(r)}\n")
        for who, cmd in (("overlap", ["-m", "vechat_amd.overlap", fq, fq]), ("cluster", ["-m", "vechat_amd.cluster", "--tsv", os.path.join(d, "c.tsv"), fq])):
            t0 = time.perf_counter()
            subprocess.run([sys.executable] + cmd, check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
            out.append((who, time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--loci", type=int, default=32)
    ap.add_argument("--locus-len", type=int, default=6000)
    ap.add_argument("--err", type=float, default=0.06)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_rate.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) the four calls under the profiler, nothing written")
    a = ap.parse_args()
    if a.child:
        measure(a)
        return 0
    reads, locus, ov, res, best = measure(a)
    n, m, st = len(reads), len(ov), res["stats"]
    sizes = np.diff(res["cl_off"].astype(np.int64))
    pure = sum(1 for c in range(st["kept"]) if len({locus[int(r)] for r in res["members"][int(res["cl_off"][c]):int(res["cl_off"][c + 1])]}) == 1)
    lines = [f"vc_cluster on {n} simulated reads of {a.read_len} bp from {a.loci} loci of {a.locus_len} bp ({a.err:.0%} errors per read, both strands); records "
             "from vc_overlap (same_set, drop_internal 1), every parameter at its default",
             f"  best of three warm calls: {best * 1e3:.2f} ms   {m / best / 1e6:.2f} M records/s   (host clock around the synchronous call, uploads and the copy back included)",
             f"  records {m}   links {st['links']}   rounds {st['rounds']}   components {st['components']}   clusters kept {st['kept']} (sizes {int(sizes.min()) if len(sizes) else 0} .. "
             f"{int(sizes.max()) if len(sizes) else 0}; {pure} hold reads of one locus only)   reads without a cluster {int((res['cluster'] == 0xFFFFFFFF).sum())}   "
             f"twisted {int(res['cl_twisted'].sum())}   reads on the reverse strand {int(res['strand'].sum())}"]
    bw = copy_bandwidth()
    edges = 2 * st["links"]
    # k_cl_init writes 2 n words; k_cl_hook reads an edge (8 bytes) and at least parent[u], parent[v] and their parents' entries (16 bytes), and
    # writes one word per hook; k_cl_flatten reads and writes 2 n words
    moved = 4 * 2 * n + edges * (8 + 16) + 4 * 2 * n + 8 * 2 * n
    if bw:
        lines.append(f"components step (k_cl_init, k_cl_hook, k_cl_flatten), expected first: {moved} bytes read plus written at the least over the {bw:.2f} TB/s of "
                     f"tools/hbm_bw.hip's copy kernel in this session = {moved / (bw * 1e12) * 1e6:.2f} us per call, were it bandwidth alone (three launches cost more "
                     "than that at this size, and the hook kernel waits on dependent loads and atomics, not on bandwidth)")
    else:
        lines.append(f"components step: {moved} bytes read plus written per call at the least; tools/hbm_bw.hip could not be run in this session, so no expected time is stated")
    rows = kernel_rows(a)
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    lines.append("kernel shares (rocprofv3 --kernel-trace --stats, a run of its own: four vc_cluster calls), among the clusterer's own kernels -- "
                 "hipcub's sort and scan kernels are left out, the run's one vc_overlap call uses the same ones:")
    for r in rows[:14]:
        lines.append(f"  {100.0 * float(r['TotalDurationNs']) / total:5.1f} %  {float(r['TotalDurationNs']) / 1e6:9.3f} ms  {int(r['Calls']):5d} calls  {r['Name'][:90]}")
    step = [r for r in rows if any(k in r["Name"] for k in ("k_cl_init", "k_cl_hook", "k_cl_flatten"))]
    if step:
        per = sum(float(r["TotalDurationNs"]) / int(r["Calls"]) for r in step)
        lines.append(f"components step, the figure: {per / 1e3:.1f} us per call over its three kernels, {moved / per:.1f} GB/s")
    lines.append("the commands on the same reads (child processes): wall seconds, process start-up, reading the FASTQ and, for the cluster command, its own "
                 "overlap call included")
    for who, dt in command_times(reads):
        lines.append(f"  {who:10s} {dt:7.2f} s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
