#!/usr/bin/env python3
"""Rate of the device scrubber (vc_scrub) on a simulated read set with spliced chimeras; writes profiles/scrub_rate.txt.

  python tools/gpu_scrub_rate.py [--reads 2000] [--read-len 5000] [--genome 1000000] [--err 0.06] [--chimeras 0.05] [--out profiles/scrub_rate.txt]

The set is the one of tools/gpu_overlap_rate.py (2 000 reads of 5 kb, 10x of a 1 Mb genome, both strands, 6 % errors per read) with
a share of the reads replaced by the first half of one read joined to the second half of another.  Reported: intervals/s and bases/s
of a warm vc_scrub call with bases and qualities (best of three, host clock around the synchronous call, uploads and the copy back
included), the classes it finds, the kernel shares from a `rocprofv3 --kernel-trace --stats` run of its own (a child process), for
k_scr_cut the time expected from the bytes it moves and the copy bandwidth tools/hbm_bw.hip reports in the same session -- stated
before the figure -- and the wall time of the scrub command beside the overlap and polish commands of one driver run on a set a
tenth the size.  There is no CPU baseline (no yacrd here) and no threshold: the file records what was measured.  Needs the GPU."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_overlap_rate import simulate  # noqa: E402


def spliced(a, n_reads=None, genome=None):
    """the simulated reads, every 1 / share-th one replaced by a chimera of itself and the read half the set away"""
    reads = simulate(n_reads or a.reads, a.read_len, genome or a.genome, a.err)
    step, n = max(int(round(1 / a.chimeras)), 1) if a.chimeras > 0 else 0, len(reads)
    made = 0
    for i in range(0, n, step) if step else ():
        other = reads[(i + n // 2) % n]
        reads[i] = reads[i][:len(reads[i]) // 2] + other[len(other) // 2:]
        made += 1
    return reads, made


def measure(a):
    from vechat_amd import overlap, scrub
    reads, made = spliced(a)
    quals = [b"5" * len(r) for r in reads]
    ov = overlap.find_overlaps(reads, None, drop_internal=0)
    iv = scrub.intervals_from_records(ov, dual=True)
    times, res = [], None
    for _ in range(4):                                          # the first call is the warm-up
        t0 = time.perf_counter()
        _, res = scrub.scrub(reads, iv, quals=quals, coverage=a.coverage)
        times.append(time.perf_counter() - t0)
    return reads, made, len(iv), res, min(times[1:])


def kernel_rows(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "scr", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--read-len", str(a.read_len),
               "--genome", str(a.genome), "--err", str(a.err), "--chimeras", str(a.chimeras), "--coverage", str(a.coverage)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    return [r for r in rows if "k_scr_" in r["Name"]]


def copy_bandwidth():
    """TB/s of the copy kernel of tools/hbm_bw.hip (its larger grid), or None when the probe cannot be built or run"""
    exe = os.path.join(ROOT, "tools", "hbm_bw.bin")
    try:
        if not os.path.exists(exe):
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", os.path.join(ROOT, "tools", "hbm_bw.hip"), "-o", exe],
                           check=True, timeout=600)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
        return max(float(x) for x in re.findall(r"^copy\s+([0-9.]+) TB/s", out, re.M))
    except (OSError, subprocess.SubprocessError, ValueError):
        return None


def driver_run(a):
    from vechat_amd import driver
    reads, _ = spliced(a, a.reads // 10, a.genome // 10)
    times, real = [], driver._sh

    def timed(cmd, cwd):
        t0 = time.perf_counter()
        real(cmd, cwd)
        times.append((next(w for w in ("scrub", "overlap", "polish") if "vechat_amd." + w in cmd), time.perf_counter() - t0))

    driver._sh = timed
    try:
        with tempfile.TemporaryDirectory() as d:
            fq = os.path.join(d, "reads.fastq")
            with open(fq, "w") as f:
                for i, r in enumerate(reads):
                    f.write(f"@r{i}\n{r.decode()}\n+\n{'5' * len(r)}\n")
            driver.main([fq, "-o", os.path.join(d, "out.fa"), "--workdir", os.path.join(d, "work"), "--overlapper", "device", "--scrub", "--scrubber", "device",
                         "--platform", "ont", "--linear", "-u"])
    finally:
        driver._sh = real
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--err", type=float, default=0.06)
    ap.add_argument("--chimeras", type=float, default=0.05, help="share of the reads spliced into chimeras")
    ap.add_argument("--coverage", type=int, default=1, help="vc_scrub's threshold c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scrub_rate.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) the four calls under the profiler, nothing written")
    a = ap.parse_args()
    if a.child:
        measure(a)
        return 0
    reads, made, m, res, best = measure(a)
    bases = sum(len(r) for r in reads)
    cut = int(res["pc_off"][-1])
    lines = [f"vc_scrub on {a.reads} simulated reads of {a.read_len} bp ({bases} bases, genome {a.genome} bp, {a.err:.0%} errors per read, both strands), "
             f"{made} of them spliced chimeras; intervals from vc_overlap (same_set, drop_internal 0), c = {a.coverage}, bases and qualities cut",
             f"  best of three warm calls: {best * 1e3:.1f} ms   {m / best / 1e6:.2f} M intervals/s   {bases / best / 1e6:.1f} Mbases/s   (host clock around the synchronous call, uploads and the copy back included)",
             f"  intervals {m}   events {res['stats']['events']}   segments {res['stats']['segments']}   regions {res['stats']['regions']}   pieces {res['stats']['pieces']}   bytes cut {cut} (x 2: bases and qualities)",
             "  classes clean / bad ends / chimeric / not covered: " + " / ".join(str(int(x)) for x in np.bincount(res["klass"], minlength=4))]
    bw = copy_bandwidth()
    moved = 4 * cut                                             # bases and qualities, each read once and written once
    if bw:
        lines.append(f"k_scr_cut, expected first: {moved} bytes read plus written over the {bw:.2f} TB/s of tools/hbm_bw.hip's copy kernel in this session = "
                     f"{moved / (bw * 1e12) * 1e6:.1f} us per call, were it bandwidth alone (a launch costs more than that at this size)")
    else:
        lines.append(f"k_scr_cut: {moved} bytes read plus written per call; tools/hbm_bw.hip could not be run in this session, so no expected time is stated")
    rows = kernel_rows(a)
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    lines.append("kernel shares (rocprofv3 --kernel-trace --stats, a run of its own: four vc_scrub calls), among the scrubber's own kernels -- "
                 "hipcub's sort and scan kernels are left out, the run's one vc_overlap call uses the same ones:")
    for r in rows[:14]:
        lines.append(f"  {100.0 * float(r['TotalDurationNs']) / total:5.1f} %  {float(r['TotalDurationNs']) / 1e6:9.3f} ms  {int(r['Calls']):5d} calls  {r['Name'][:90]}")
    for r in rows:
        if "k_scr_cut" in r["Name"]:
            per = float(r["TotalDurationNs"]) / int(r["Calls"])
            lines.append(f"k_scr_cut, the figure: {per / 1e3:.1f} us per call, {moved / per:.1f} GB/s")
    lines.append(f"one driver run (--linear --overlapper device --scrub --scrubber device, child processes) on {a.reads // 10} reads of a {a.genome // 10} bp genome "
                 "(the same coverage): wall seconds per command, process start-up included")
    for who, dt in driver_run(a):
        lines.append(f"  {who:10s} {dt:7.2f} s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
