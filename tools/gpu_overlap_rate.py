#!/usr/bin/env python3
"""Rate of the device overlapper (vc_overlap) on a simulated read set; writes profiles/overlap_rate.txt.

  python tools/gpu_overlap_rate.py [--reads 2000] [--read-len 5000] [--genome 1000000] [--err 0.06] [--out profiles/overlap_rate.txt]

The set stands for one driver chunk: 2 000 reads of 5 kb (10 Mb, 10x of a 1 Mb genome, both strands, 6 % errors per read).
Reported: reads/s and bases/s of find_overlaps (warm, best of three, host clock around the synchronous call), the minimizers,
anchors and chains of the call, the kernel shares from a `rocprofv3 --kernel-trace --stats` run of its own (a child process),
and the wall time of the overlapper command beside the polisher command in one driver round on a set a tenth the size.
There is no CPU baseline (no minimap2 here) and no threshold: the file records what was measured.  Needs the GPU."""
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
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def simulate(n_reads, read_len, genome_len, err, seed=3):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    g = rng.choice(alpha, genome_len)
    reads = []
    for i in range(n_reads):
        s = int(rng.integers(0, genome_len - read_len + 1))
        src = g[s:s + read_len]
        r = rng.random(read_len)
        keep = r >= err * 0.3                                   # deletions
        sub = (r >= err * 0.7) & (r < err)                      # substitutions
        out = np.where(sub, alpha[(np.searchsorted(alpha, src) + rng.integers(1, 4, read_len)) % 4], src)
        ins = (r >= err * 0.3) & (r < err * 0.7)                # an inserted base in front
        parts = np.stack([np.where(ins, rng.choice(alpha, read_len), 0), out])
        flat = parts.T[keep].reshape(-1)
        seq = flat[flat != 0].astype(np.uint8).tobytes()
        reads.append(seq if i % 2 else seq.translate(COMP)[::-1])
    return reads


def measure(a):
    from vechat_amd import overlap
    reads = simulate(a.reads, a.read_len, a.genome, a.err)
    bases = sum(len(r) for r in reads)
    stats, times, n = {}, [], 0
    for _ in range(4):                                          # the first call is the warm-up
        t0 = time.perf_counter()
        n = len(overlap.find_overlaps(reads, stats=stats))
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    return reads, bases, stats, best, n


def kernel_shares(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "ovl", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--read-len", str(a.read_len),
               "--genome", str(a.genome), "--err", str(a.err)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    return [(r["Name"][:90], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, 100.0 * float(r["TotalDurationNs"]) / total) for r in rows[:12]]


def driver_round(reads):
    from vechat_amd import driver
    times = []
    real = driver._sh

    def timed(cmd, cwd):
        t0 = time.perf_counter()
        real(cmd, cwd)
        times.append(("overlapper" if "vechat_amd.overlap" in cmd else "polisher", time.perf_counter() - t0))

    driver._sh = timed
    try:
        with tempfile.TemporaryDirectory() as d:
            fq = os.path.join(d, "reads.fastq")
            with open(fq, "w") as f:
                for i, r in enumerate(reads):
                    f.write(f"@r{i}\n{r.decode()}\n+\n{'5' * len(r)}\n")
            driver.main([fq, "-o", os.path.join(d, "out.fa"), "--workdir", os.path.join(d, "work"), "--overlapper", "device", "--platform", "ont", "--linear", "-u"])
    finally:
        driver._sh = real
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--err", type=float, default=0.06)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_rate.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) one warm call and one traced call, nothing written")
    a = ap.parse_args()
    if a.child:
        measure(a)
        return 0
    reads, bases, stats, best, n = measure(a)
    lines = [f"vc_overlap on {a.reads} simulated reads of {a.read_len} bp ({bases} bases, genome {a.genome} bp, {a.err:.0%} errors per read, both strands), same_set, defaults",
             f"  best of three warm calls: {best * 1e3:.1f} ms   {a.reads / best:.0f} reads/s   {bases / best / 1e6:.1f} Mbases/s   (host clock around the synchronous call, uploads and the record copy included)",
             f"  minimizers {stats['minimizers']}   anchors {stats['anchors']}   chains (keys) {stats['keys']}   records {n}"]
    lines.append("kernel shares (rocprofv3 --kernel-trace --stats, a run of its own: four calls):")
    for name, calls, ms, pct in kernel_shares(a):
        lines.append(f"  {pct:5.1f} %  {ms:9.2f} ms  {calls:5d} calls  {name}")
    lines.append(f"one driver round (--linear --overlapper device, child processes) on {a.reads // 10} reads of a {a.genome // 10} bp genome (the same coverage): "
                 "wall seconds per command, process start-up included")
    for who, dt in driver_round(simulate(a.reads // 10, a.read_len, a.genome // 10, a.err)):
        lines.append(f"  {who:10s} {dt:7.2f} s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
