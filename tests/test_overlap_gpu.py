"""The overlapper on the device, pinned to the CPU restatement of its rule (tests/overlap_ref.py) array for array: the hand-built
cases of tests/overlap_cases.py, a simulated read set with the default budget and cut into target pieces, every class of k and w
(hashes of 8 to 56 bits), reads full of tandem repeats, a seeded sweep over all parameters, many calls in one process, the command
line with two files, identity() against the aligner's CPU DP, and one run of the two-round driver that never leaves the device
for its overlaps."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_ref
import overlap_cases as OC
import overlap_ref as R
from test_driver import _fit_distance, simulate
import test_overlap as TO
from test_overlap import simulated
from vechat_amd import capi, driver, overlap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def same_records(got, want):
    assert got.dtype == want.dtype
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), (f, got[f][:8], want[f][:8])


@pytest.mark.parametrize("name", sorted(OC.SKETCH_CASES))
def test_sketch_equals_the_restatement(built, name):
    seqs, k, w, expect = OC.SKETCH_CASES[name]
    got, want = overlap.sketch(seqs, k=k, w=w), R.sketch(seqs, k, w)
    same_records(got, want)
    if expect is not None:
        assert [(int(s), int(p)) for s, p in zip(got["seq"], got["pos"])] == expect


def pieces(capfd):
    return [int(m) for m in re.findall(r"vc_overlap: piece first=\d+ targets=(\d+) ", capfd.readouterr().err)]


@pytest.mark.parametrize("name", sorted(OC.OVERLAP_CASES))
def test_overlaps_equal_the_restatement(built, name, monkeypatch, capfd):
    c = OC.OVERLAP_CASES[name]
    monkeypatch.setenv("VC_OVL_LOG", "1")
    if c["budget_mb"] is not None:
        monkeypatch.setenv("VC_OVL_BUDGET_MB", str(c["budget_mb"]))
    else:
        monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
    stats = {}
    got = overlap.find_overlaps(c["targets"], c["queries"], stats=stats, **c["params"])
    per_piece = pieces(capfd)
    want = R.overlaps(c["targets"], c["queries"], **c["params"])
    same_records(got, want)
    if c["expect"] is not None:
        assert [tuple(int(x) for x in r) for r in got] == c["expect"]
    P = dict(R.DEFAULTS, **c["params"])
    same = c["queries"] is None
    keys = R.seeds(c["targets"], c["targets"] if same else c["queries"], P["k"], P["w"], P["max_occ"], 1 if same else 0)
    assert stats["anchors"] == sum(len(a) for a in keys.values()) and stats["keys"] == len(keys)
    assert len(per_piece) >= c["min_pieces"] and sum(per_piece) == (len(c["targets"]) if stats["minimizers"] else 0)


def test_simulated_reads_equal_the_restatement_whole_and_in_pieces(built, monkeypatch, capfd):
    seqs, _, want = simulated(0.06)
    monkeypatch.setenv("VC_OVL_LOG", "1")
    monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
    same_records(overlap.find_overlaps(list(seqs)), want)
    assert len(pieces(capfd)) == 1 and len(want) > 700
    monkeypatch.setenv("VC_OVL_BUDGET_MB", "0.25")          # 4 681 anchors a piece
    same_records(overlap.find_overlaps(list(seqs)), want)
    cut = pieces(capfd)
    assert len(cut) >= 3 and sum(cut) == len(seqs)
    # the same reads as two sets: every pair of the one-set run, and every read against itself
    monkeypatch.delenv("VC_OVL_BUDGET_MB")
    two = overlap.find_overlaps(list(seqs[:20]), list(seqs[:20]))
    same_records(two, R.overlaps(list(seqs[:20]), list(seqs[:20])))
    assert sum(1 for r in two if r["q_id"] == r["t_id"] and r["strand"] == 0) == 20


def same_counts(stats, keys):
    assert stats["anchors"] == sum(len(a) for a in keys.values()) and stats["keys"] == len(keys)


@pytest.mark.parametrize("k,w", TO.CLASSES)
def test_every_k_and_w_class_equals_the_restatement(built, k, w, monkeypatch, capfd):
    """hashes of 8 bits (k 4: a few buckets, all beyond max_occ or nearly), of exactly 32 (k 16), of 34, 38 and 56 (k 17, 19, 28), every
    k-mer a minimizer (w 1) and the widest window (w 64): the minimizer table, the records and the seed counters"""
    tab, want, keys = TO.class_preconditions(k, w)
    seqs = list(TO.sixteen_reads())
    monkeypatch.setenv("VC_OVL_LOG", "1")
    monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
    same_records(overlap.sketch(seqs, k=k, w=w), tab)
    stats = {}
    same_records(overlap.find_overlaps(seqs, None, stats=stats, k=k, w=w, min_overlap=300), want)
    same_counts(stats, keys)
    assert stats["minimizers"] == len(tab) and len(pieces(capfd)) == 1
    if (k, w) == (19, 5):                                    # the product's preset once more, cut into target pieces
        monkeypatch.setenv("VC_OVL_BUDGET_MB", "0.05")       # 936 anchors a piece
        stats = {}
        same_records(overlap.find_overlaps(seqs, None, stats=stats, k=k, w=w, min_overlap=300), want)
        same_counts(stats, keys)
        cut = pieces(capfd)
        assert len(cut) >= 3 and sum(cut) == len(seqs)


@pytest.mark.parametrize("max_occ", (100, 20))
def test_repeat_reads_equal_the_restatement(built, max_occ, monkeypatch):
    """reads across 30 copies of a 37-base unit: buckets at and beyond max_occ, a key of thousands of anchors with most of them off
    the diagonal, anchors that share their t_pos -- and max_occ decides which records there are"""
    TO.repeat_preconditions()
    monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
    want, keys = TO.restated_repeats(max_occ)
    stats = {}
    same_records(overlap.find_overlaps(OC.repeat_reads(), None, stats=stats, min_overlap=300, max_occ=max_occ), want)
    same_counts(stats, keys)


@pytest.mark.parametrize("part", range(4))
def test_seeded_sweep_equals_the_restatement(built, part, monkeypatch):
    """24 configurations from one seed (overlap_cases.sweep; tests/test_overlap.py holds them to >= 16 with records and >= 200 records),
    six a part: the minimizer tables, the records and the seed counters.  Every mismatch of a part is reported, not the first."""
    cs, res = OC.sweep(), TO.restated_sweep()
    bad = []
    for i in range(6 * part, 6 * part + 6):
        c, (want, anchors, keys, tabs) = cs[i], res[i]
        if c["budget_mb"] is None:
            monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
        else:
            monkeypatch.setenv("VC_OVL_BUDGET_MB", str(c["budget_mb"]))
        stats = {}
        got = overlap.find_overlaps(c["targets"], c["queries"], stats=stats, **c["params"])
        sk = [overlap.sketch(s, k=c["params"]["k"], w=c["params"]["w"]) for s in ((c["targets"],) if c["queries"] is None else (c["targets"], c["queries"]))]
        why = []
        if got.dtype != want.dtype or len(got) != len(want) or any(not np.array_equal(got[f], want[f]) for f in want.dtype.names):
            why.append(("records", len(got), len(want)))
        if (stats["anchors"], stats["keys"]) != (anchors, keys):
            why.append(("counters", stats["anchors"], stats["keys"], anchors, keys))
        if any(a.dtype != b.dtype or len(a) != len(b) or any(not np.array_equal(a[f], b[f]) for f in b.dtype.names) for a, b in zip(sk, tabs)):
            why.append(("sketch", [len(a) for a in sk], [len(b) for b in tabs]))
        if why:
            bad.append((i, c["params"], c["queries"] is None, c["budget_mb"], why))
    assert not bad, bad


def test_many_calls_in_one_process(built, monkeypatch):
    """The library keeps one set of result arrays a process: a small answer after a large one, an empty one, a sketch in between,
    a call after vc_overlap_release() -- each equal to the restatement in length and content, the first and the last to each other."""
    monkeypatch.delenv("VC_OVL_BUDGET_MB", raising=False)
    seqs = list(TO.sixteen_reads())
    tab, want, _ = TO.class_preconditions(19, 5)
    first = overlap.find_overlaps(seqs, None, k=19, w=5, min_overlap=300)
    assert len(first) == len(want) >= 50
    same_records(first, want)
    small, none = OC.OVERLAP_CASES["block_of_500_and_499"], OC.OVERLAP_CASES["bucket_of_one_sequence_only"]
    got = overlap.find_overlaps(small["targets"], small["queries"], **small["params"])
    assert [tuple(int(x) for x in r) for r in got] == small["expect"] and len(got) == 1
    same_records(got, R.overlaps(small["targets"], small["queries"], **small["params"]))
    got = overlap.find_overlaps(none["targets"], none["queries"], **none["params"])
    assert none["expect"] == [] and len(got) == 0
    same_records(got, R.overlaps(none["targets"], none["queries"], **none["params"]))
    sk = overlap.sketch(seqs, k=19, w=5)
    assert len(sk) == len(tab) > 0
    same_records(sk, tab)
    overlap.declare(capi.load_hip()).vc_overlap_release()
    last = overlap.find_overlaps(seqs, None, k=19, w=5, min_overlap=300)
    assert len(last) == len(want)
    same_records(last, want)
    same_records(last, first)


def test_command_line_with_two_files_ava_pb(built, tmp_path):
    """`python -m vechat_amd.overlap -x ava-pb` as a process of its own, with two different files and --min-identity and with one file
    twice: stdout is, byte for byte, the PAF text tests/test_overlap.py works out from the restatement and the aligner's CPU DP."""
    want = TO.command_line_preconditions()
    targets, reads = TO.command_line_files()
    for name, recs in (("targets.fa", targets), ("reads.fa", reads)):
        (tmp_path / name).write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in recs))
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    env.pop("VC_OVL_BUDGET_MB", None)
    for args, text in zip(TO.CLI_ARGS, want):
        p = subprocess.run([sys.executable, "-m", "vechat_amd.overlap", *args], cwd=tmp_path, env=env, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout == text.encode(), (args, p.stdout.decode().splitlines()[:3], text.splitlines()[:3])


def test_identity_against_the_cpu_dp(built):
    seqs, _, want = simulated(0.06)
    picks = want[[0, 1, len(want) // 2, len(want) - 1]]
    assert picks["strand"].any() and not picks["strand"].all()
    got = overlap.identity(picks, list(seqs))
    for g, r in zip(got, picks):
        q = seqs[int(r["q_id"])][int(r["q_begin"]):int(r["q_end"])]
        if r["strand"]:
            q = q.translate(_COMP)[::-1]
        cigar, dist = align_ref.align(q, seqs[int(r["t_id"])][int(r["t_begin"]):int(r["t_end"])])
        cols = sum(int(x) for x in re.findall(r"(\d+)[MID]", cigar))
        assert (int(g["block"]), int(g["matches"])) == (cols, cols - dist)
        assert all(g[f] == r[f] for f in ("q_id", "t_id", "strand", "q_begin", "q_end", "t_begin", "t_end", "n_anchors", "score"))
        assert 0.8 < int(g["matches"]) / int(g["block"]) < 1.0            # two reads with 6 % errors each


def test_both_rounds_with_the_device_overlapper(built, tmp_path, monkeypatch):
    """tests/test_driver.py::test_both_rounds_on_the_device with `--overlapper device` in place of the stub: the same reads, the same
    acceptance, and no command but this package's own (the ont preset, k = 15: at 10 % errors per read two reads share one 19-mer in
    seventy; round 2 keeps overlaps of 90 % identity, where the stub test applies no identity filter at all)."""
    reads = tmp_path / "reads.fastq"
    recs, truth = simulate(str(reads), n_reads=16, genome_len=2400, read_len=1500, err=0.10, seed=9)
    out = tmp_path / "out.fa"
    log = []
    monkeypatch.setattr(driver, "COMMAND_LOG", log)
    rc = driver.main([str(reads), "-o", str(out), "--workdir", str(tmp_path / "work"), "--overlapper", "device", "--platform", "ont",
                      "--min-ovlplen-cns", "400", "--min-identity-cns", "0.9", "-u"])
    assert rc == 0
    assert len(log) == 4 and all("stub" not in c and "minimap2" not in c for c in log) and sum("vechat_amd.overlap" in c for c in log) == 2
    lines = open(out).read().split("\n")
    got = {lines[i][1:].split()[0].rstrip("r"): lines[i + 1].encode() for i in range(0, len(lines) - 1, 2)}    # one 'r' per round
    assert set(got) == {n for n, _ in recs}
    picks = recs[:6]
    before = sum(_fit_distance(s, truth[n]) for n, s in picks) / sum(len(s) for _, s in picks)
    after = sum(_fit_distance(got[n], truth[n]) for n, _ in picks) / sum(len(got[n]) for n, _ in picks)
    assert all(len(got[n]) > 0.7 * len(truth[n]) for n, _ in picks)
    assert after * 3 < before, (before, after)               # ~10 % raw error rate
    for n, s in picks:                                       # every read ends closer to its haplotype than it started
        assert _fit_distance(got[n], truth[n]) / len(got[n]) < _fit_distance(s, truth[n]) / len(s), n
