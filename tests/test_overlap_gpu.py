"""The overlapper on the device, pinned to the CPU restatement of its rule (tests/overlap_ref.py) array for array: the hand-built
cases of tests/overlap_cases.py, a simulated read set with the default budget and cut into target pieces, identity() against
the aligner's CPU DP, and one run of the two-round driver that never leaves the device for its overlaps."""
import os
import re

import numpy as np
import pytest

import align_ref
import overlap_cases as OC
import overlap_ref as R
from test_driver import _fit_distance, simulate
from test_overlap import simulated
from vechat_amd import driver, overlap

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
