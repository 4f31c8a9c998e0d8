#!/usr/bin/env python3
"""Rate of the device demultiplexer (vc_demux) on simulated barcoded reads; writes profiles/demux_rate.txt.

  python tools/gpu_demux_rate.py [--reads 200000] [--read-len 2000] [--patterns 96] [--pattern-len 24] [--out profiles/demux_rate.txt]

The set: seeded barcodes, every read with its barcode in front and the barcode's reverse complement behind, on a random strand, 5 %
substitutions.  Reported: ms per warm vc_demux call with qualities and ORIENT (best of three, host clock around the synchronous call,
uploads and the copy back included), reads/s, pattern-character steps/s (2 views x min(len, window) characters x patterns per read),
the kernel shares from a `rocprofv3 --kernel-trace --stats` run of its own (a child process), the vector instructions of
k_dmx_search per step counted from its ISA beside the integer issue rate that vechat_amd/lib/valu_peak.bin measures in the same
session, and k_dmx_cut against the copy bandwidth of tools/hbm_bw.hip.  There is no CPU baseline (no cutadapt here) and no pass
mark.  The expectation, stated before the figures: the search kernel is issue-bound -- its time is steps x instructions per step
over the issue rate, within the spread between sessions that profiles/overlap_rate.txt shows.  Needs the GPU."""
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
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def simulate(a):
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    barcodes = [rng.choice(acgt, a.pattern_len).tobytes() for _ in range(a.patterns)]
    reads = []
    for _ in range(a.reads):
        b = barcodes[int(rng.integers(a.patterns))]
        body = np.concatenate([np.frombuffer(b, np.uint8), rng.choice(acgt, max(a.read_len - 2 * a.pattern_len, 0)), np.frombuffer(b.translate(COMP)[::-1], np.uint8)])
        hit = rng.random(len(body)) < 0.05
        body[hit] = rng.choice(acgt, int(hit.sum()))
        r = body.tobytes()
        reads.append(r.translate(COMP)[::-1] if rng.random() < 0.5 else r)
    return barcodes, reads


def measure(a):
    from vechat_amd import demux
    barcodes, reads = simulate(a)
    quals = [b"5" * len(r) for r in reads]
    times, res = [], None
    for _ in range(4):                                          # the first call is the warm-up
        t0 = time.perf_counter()
        res = demux.demux_reads(reads, barcodes, quals=quals, orient=True, window=a.window)
        times.append(time.perf_counter() - t0)
    return reads, res, min(times[1:])


def kernel_rows(a):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "dmx", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--read-len", str(a.read_len),
               "--patterns", str(a.patterns), "--pattern-len", str(a.pattern_len), "--window", str(a.window)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    return [r for r in rows if "k_dmx_" in r["Name"]]


def search_valu_per_step():
    """vector instructions of k_dmx_search's inner loop per character: the v_ instructions from its LDS word read to the branch that
    closes the loop, over the four characters of a word; None when the library cannot be disassembled"""
    import isa_lint
    llvm, magic, dis = isa_lint.LLVM, b"__CLANG_OFFLOAD_BUNDLE__", ""
    try:
        with tempfile.TemporaryDirectory() as tmp:
            # the library's fat binary holds one offload bundle per translation unit, back to back: take them apart at the magic
            fat = os.path.join(tmp, "fat.bin")
            subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", os.path.join(ROOT, "vechat_amd", "lib", "libvechat_hip.so"), fat])
            data = open(fat, "rb").read()
            for k, part in enumerate(data.split(magic)[1:]):
                if b"k_dmx_search" not in part:
                    continue
                one, co = os.path.join(tmp, f"b{k}.bin"), os.path.join(tmp, f"b{k}.co")
                open(one, "wb").write(magic + part)
                targets = subprocess.check_output([os.path.join(llvm, "clang-offload-bundler"), "--list", "--type=o", "--input=" + one]).decode().split()
                tgt = next(t for t in targets if "gfx950" in t)
                subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + one, "--targets=" + tgt, "--output=" + co])
                dis = subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", "--symbolize-operands", co]).decode("utf-8", "replace")
    except (OSError, subprocess.SubprocessError, StopIteration):
        return None
    m = re.search(r"<[^>\n]*k_dmx_search[^>\n]*>:\n(.*?)(\n[0-9a-f]+ <(?!L\d+>)|\Z)", dis, re.S)
    if not m:
        return None
    ops, labels = [], {}
    for line in m.group(1).split("\n"):
        lab = re.match(r"[0-9a-f\s]*<(L\d+)>:", line)
        if lab:
            labels[lab.group(1)] = len(ops)
            continue
        p = isa_lint.parse(line)
        if p:
            ops.append(p)
    # the innermost loop around the LDS word read: from the label a later branch jumps back to, to that branch
    for i, (op, _) in enumerate(ops):
        if op == "ds_read_b32":
            for j in range(i + 1, len(ops)):
                back = labels.get(ops[j][1][-1].strip("<>")) if ops[j][0].startswith("s_cbranch") and ops[j][1] else None
                if back is not None and back <= i:
                    return sum(1 for o, _ in ops[back:j] if o.startswith("v_")) / 4.0
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--read-len", type=int, default=2000)
    ap.add_argument("--patterns", type=int, default=96)
    ap.add_argument("--pattern-len", type=int, default=24)
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demux_rate.txt"))
    ap.add_argument("--child", action="store_true", help="(internal) the four calls under the profiler, nothing written")
    a = ap.parse_args()
    if a.child:
        measure(a)
        return 0
    from gpu_scrub_rate import copy_bandwidth
    import bench
    reads, res, best = measure(a)
    steps = sum(2 * min(len(r), a.window) for r in reads) * a.patterns
    cut = int(res["piece_off"][-1])
    lines = [f"vc_demux on {a.reads} simulated reads of {a.read_len} bp, {a.patterns} barcodes of {a.pattern_len} bases on both ends, 5 % substitutions, random strand; "
             f"window {a.window}, defaults, qualities, ORIENT",
             "expected first: k_dmx_search is issue-bound -- its time is steps x vector instructions per step over the integer issue rate of this session, "
             "within the spread between sessions that profiles/overlap_rate.txt shows; no pass mark",
             f"  best of three warm calls: {best * 1e3:.1f} ms   {a.reads / best / 1e6:.3f} M reads/s   {steps / best / 1e9:.2f} G pattern-character steps/s   "
             "(host clock around the synchronous call, uploads and the copy back included)",
             f"  triples {res['stats']['triples']}   pieces of the budget {res['stats']['pieces']}   accepted hits {res['stats']['accepted']}   bytes cut {cut} (x 2: bases and qualities)",
             "  classes none / one end / both ends / conflict / ambiguous: " + " / ".join(str(int(x)) for x in np.bincount(res["klass"], minlength=5))]
    rows = kernel_rows(a)
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    lines.append("kernel shares (rocprofv3 --kernel-trace --stats, a run of its own: four vc_demux calls), among the demultiplexer's own kernels:")
    for r in rows:
        lines.append(f"  {100.0 * float(r['TotalDurationNs']) / total:5.1f} %  {float(r['TotalDurationNs']) / 1e6:9.3f} ms  {int(r['Calls']):5d} calls  {r['Name'][:90]}")
    per_step = search_valu_per_step()
    peak = bench.valu_peak_now(0)
    rate = (peak["classes"].get("i32_max_add") or {}).get("inst_per_us_per_simd") or peak.get("pk16")      # 32-bit integer VALU, else the packed 16-bit chain
    for r in rows:
        per = float(r["TotalDurationNs"]) / int(r["Calls"])
        if "k_dmx_search" in r["Name"]:
            lines.append(f"k_dmx_search, the figure: {per / 1e6:.3f} ms per call, {steps / per:.2f} G steps/s; {per_step} vector instructions per step from its ISA; "
                         f"issue rate of this session {rate} inst/us/SIMD ({peak['source']})")
            if per_step and rate:
                bound = steps / 64.0 * per_step / (rate * 1024.0) * 1e3          # wave instructions over 256 CUs x 4 SIMDs, in ns
                lines.append(f"  issue-bound time for these steps: {bound / 1e6:.3f} ms ({100.0 * bound / per:.0f} % of the figure)")
        if "k_dmx_cut" in r["Name"]:
            bw = copy_bandwidth()
            lines.append(f"k_dmx_cut, the figure: {per / 1e3:.1f} us per call, {4 * cut / per:.1f} GB/s read plus written" +
                         (f"; tools/hbm_bw.hip's copy kernel in this session: {bw:.2f} TB/s" if bw else "; tools/hbm_bw.hip could not be run in this session"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
