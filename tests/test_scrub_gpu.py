"""The scrubber on the device, pinned to the CPU restatement of its rule (tests/scrub_ref.py) array for array -- regions, offsets,
classes, totals, pieces and cut bytes: the hand-built cases of tests/scrub_cases.py in the order given, reversed and shuffled, with
and without bases and qualities, a seeded sweep over all parameters, many calls in one process, the command line on simulated
reads, and one run of the driver that scrubs, overlaps and corrects without leaving this package."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import overlap_ref as OR
import scrub_cases as SC
import scrub_ref as R
import test_scrub as TS
from test_driver import simulate
from vechat_amd import capi, driver, scrub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
ARRAYS = ("reg_read", "reg_begin", "reg_end", "reg_off", "klass", "bad_total", "pc_read", "pc_begin", "pc_end", "pc_off")


def same(got, want):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (f, got[f][:8], want[f][:8])
    for f in ("pc_bases", "pc_quals"):
        assert got[f] == want[f], (f, None if got[f] is None else len(got[f]), None if want[f] is None else len(want[f]))


def logged(capfd):
    return [tuple(int(x) for x in m) for m in re.findall(r"vc_scrub: intervals=(\d+) events=(\d+) segments=(\d+) regions=(\d+) pieces=(\d+)", capfd.readouterr().err)]


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_cases_equal_the_restatement(built, name, monkeypatch, capfd):
    c, want = SC.CASES[name], TS.restated(name)
    reads, quals = SC.reads_of(c["lengths"])
    monkeypatch.setenv("VC_SCRUB_LOG", "1")
    got = scrub.run(c["lengths"], c["intervals"], reads, quals, **c["params"])
    same(got, want)
    if c["expect"] is not None:
        assert TS.triples(got, "reg") == c["expect"]["regions"] and TS.triples(got, "pc") == c["expect"]["pieces"]
        assert [int(k) for k in got["klass"]] == c["expect"]["klass"] and [int(t) for t in got["bad_total"]] == c["expect"]["bad_total"]
    m = len(c["intervals"])
    (li, le, ls, lr, lp), = logged(capfd)
    assert (li, le, lr, lp) == (m, 2 * m, len(want["reg_read"]), len(want["pc_read"])) and ls <= le
    assert got["stats"] == dict(intervals=m, events=2 * m, segments=ls, regions=lr, pieces=lp)
    # the intervals reversed and shuffled; bases without qualities; neither
    order = np.random.default_rng(4).permutation(m)
    same(scrub.run(c["lengths"], c["intervals"][::-1], reads, quals, **c["params"]), want)
    same(scrub.run(c["lengths"], [c["intervals"][i] for i in order], reads, None, **c["params"]), dict(want, pc_quals=None))
    same(scrub.run(c["lengths"], c["intervals"], **c["params"]), dict(want, pc_bases=None, pc_quals=None))


@pytest.mark.parametrize("part", range(3))
def test_seeded_sweep_equals_the_restatement(built, part):
    """36 configurations from one seed (scrub_cases.sweep; tests/test_scrub.py holds them to all four classes and every parameter
    value), twelve a part.  Every mismatch of a part is reported, not the first."""
    cs, res = SC.sweep(), TS.restated_sweep()
    bad = []
    for i in range(12 * part, 12 * part + 12):
        c, want = cs[i], res[i]
        reads, quals = SC.reads_of(c["lengths"], seed=2)
        got = scrub.run(c["lengths"], c["intervals"], reads if c["with_reads"] else None, quals if c["with_quals"] else None, **c["params"])
        why = [f for f in ARRAYS if got[f].dtype != want[f].dtype or not np.array_equal(got[f], want[f])] + [f for f in ("pc_bases", "pc_quals") if got[f] != want[f]]
        if why:
            bad.append((i, c["params"], why))
    assert not bad, bad


def test_many_calls_in_one_process(built):
    """The library keeps one set of result arrays a process: sizes that grow and shrink, an empty set, a call after
    vc_scrub_release() -- each equal to the restatement, the first and the last to each other."""
    names = ("one_read_with_thousands_of_intervals", "length_1_reads", "cut_every_residue_and_length", "no_interval_at_all",
             "adjacent_bad_segments_across_block_boundaries", "region_inside_alone", "one_read_with_thousands_of_intervals")
    first = None
    for i, name in enumerate(names):
        c = SC.CASES[name]
        reads, quals = SC.reads_of(c["lengths"])
        if i == len(names) - 1:
            scrub.declare(capi.load_hip()).vc_scrub_release()
        got = scrub.run(c["lengths"], c["intervals"], reads, quals, **c["params"])
        same(got, TS.restated(name))
        first = first or got
        if i == 3:                                           # no read at all, between two calls that have some
            empty = scrub.run([], [])
            assert all(len(empty[f]) == 0 for f in ARRAYS if not f.endswith("_off")) and empty["reg_off"].tolist() == [0] and empty["pc_off"].tolist() == [0]
    same(got, first)


def test_bad_regions_and_scrub(built):
    """the two public calls on a case whose answer is written out by hand"""
    c = SC.CASES["region_left_right_inside_and_all_three"]
    reg, klass, total = scrub.bad_regions(c["lengths"], c["intervals"])
    assert reg.dtype == scrub.REGION and [tuple(int(x) for x in r) for r in reg] == c["expect"]["regions"]
    assert klass.tolist() == c["expect"]["klass"] and total.tolist() == c["expect"]["bad_total"]
    _, klass, _ = scrub.bad_regions(c["lengths"], c["intervals"], max_bad_permille=399)
    assert klass.tolist() == [1, 1, 2, 3]                    # 1000 * 40 > 399 * 100
    c = SC.CASES["not_covered_read_between_two_kept_ones"]
    reads, quals = SC.reads_of(c["lengths"])
    pieces, rep = scrub.scrub(reads, c["intervals"], quals=quals)
    assert pieces == [(None, reads[0], quals[0]), (None, reads[2], quals[2])] and rep["pc_read"].tolist() == [0, 2]
    c = SC.CASES["min_piece_drops_a_short_middle_piece"]
    reads, _ = SC.reads_of(c["lengths"])
    pieces, rep = scrub.scrub(reads, c["intervals"], min_piece=10)
    assert pieces == [("_0_30", reads[0][:30], None), ("_60_100", reads[0][60:], None)] and rep["klass"].tolist() == [2]
    with pytest.raises(RuntimeError, match="outside its read"):
        scrub.bad_regions([10], [(0, 5, 11)])


# ------------------------------------------------------------------------------------------------- the command line
CLI = dict(n_reads=12, genome_len=2400, read_len=1200, err=0.02, seed=5)
CLI_ARGS = ("-x", "ava-pb", "-c", "1", "-n", "0.4", "-g", "500", "--min-piece", "50")


def command_line_expected(recs, fastq, dual=True):
    """the scrubbed text and the report of CLI_ARGS, from the two restatements alone"""
    names, reads = [n for n, _ in recs], [s for _, s in recs]
    quals = [b"5" * len(s) for s in reads] if fastq else None
    ov = OR.overlaps(reads, None, k=19, w=5, drop_internal=0, max_gap=500)
    rows = [tuple(int(r[f]) for f in ("q_id", "q_begin", "q_end", "t_id", "t_begin", "t_end")) for r in ov]
    res = R.scrub([len(s) for s in reads], R.intervals_of(rows, dual=True), reads, quals, coverage=1, max_bad_permille=400, min_piece=50)
    return R.format_reads(names, names, reads, quals, res), R.format_report(names, [len(s) for s in reads], res), res, ov


def test_command_line_on_simulated_reads(built, tmp_path):
    """`python -m vechat_amd.scrub` as a process of its own on a two-strand simulated FASTQ: the scrubbed reads and the report are,
    byte for byte, what the restatements of the overlapper and the scrubber give; then in this process with --paf (each pair once,
    as minimap2 writes it without --dual=yes) and on the same reads as FASTA."""
    recs, _ = simulate(str(tmp_path / "reads.fq"), **CLI)
    text, report, res, ov = command_line_expected(recs, True)
    assert {n.rsplit("_", 1)[1] for n, _ in recs} == {"+", "-"}
    assert len(res["pc_read"]) >= 6 and any(b > 0 or e < len(recs[r][1]) for r, b, e in TS.triples(res, "pc")) and report      # something is cut
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    p = subprocess.run([sys.executable, "-m", "vechat_amd.scrub", *CLI_ARGS, "--report", "report.txt", "-o", "out.fq", "reads.fq"], cwd=tmp_path, env=env,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert (tmp_path / "out.fq").read_text() == text and (tmp_path / "report.txt").read_text() == report
    # each pair once in a PAF file: both sides of a record count, and the answer is the same
    names = [n for n, _ in recs]
    with open(tmp_path / "half.paf", "w") as fw:
        for r in ov:
            if int(r["q_id"]) < int(r["t_id"]):
                q, t = int(r["q_id"]), int(r["t_id"])
                mirror = [x for x in ov if int(x["q_id"]) == t and int(x["t_id"]) == q and x["strand"] == r["strand"]]
                assert len(mirror) == 1                          # same_set holds (i, j) and (j, i) both
                fw.write("\t".join(str(x) for x in (names[q], len(recs[q][1]), int(r["q_begin"]), int(r["q_end"]), "-" if r["strand"] else "+", names[t],
                                                    len(recs[t][1]), int(mirror[0]["q_begin"]), int(mirror[0]["q_end"]), 0, 0, 255)) + "\n")
    buf = io.StringIO()
    assert scrub.main([*CLI_ARGS, "--paf", str(tmp_path / "half.paf"), str(tmp_path / "reads.fq")], out=buf) == 0 and buf.getvalue() == text
    simulate(str(tmp_path / "reads.fa"), fastq=False, **CLI)
    buf = io.StringIO()
    assert scrub.main([*CLI_ARGS, str(tmp_path / "reads.fa")], out=buf) == 0 and buf.getvalue() == command_line_expected(recs, False)[0]
    (tmp_path / "other.paf").write_text("nobody\t100\t0\t50\t+\t%s\t1200\t0\t50\t0\t0\t255\n" % names[0])
    with pytest.raises(ValueError, match="not a read"):
        scrub.main([*CLI_ARGS, "--paf", str(tmp_path / "other.paf"), str(tmp_path / "reads.fq")], out=io.StringIO())


# -------------------------------------------------------------------------------------------------------- driver
def test_driver_scrubs_overlaps_and_corrects_on_the_device(built, tmp_path, monkeypatch):
    """`driver --overlapper device --scrub --scrubber device --linear` on the reads of test_both_rounds_with_the_device_overlapper: three
    commands, all this package's own, a scrubbed FASTQ, a report, and a corrected FASTA of reads or pieces of reads of the input."""
    reads = tmp_path / "reads.fastq"
    recs, _ = simulate(str(reads), n_reads=16, genome_len=2400, read_len=1500, err=0.10, seed=9)
    out, work = tmp_path / "out.fa", tmp_path / "work"
    log = []
    monkeypatch.setattr(driver, "COMMAND_LOG", log)
    rc = driver.main([str(reads), "-o", str(out), "--workdir", str(work), "--overlapper", "device", "--scrub", "--scrubber", "device", "--platform", "ont",
                      "--linear", "-u"])
    assert rc == 0
    assert len(log) == 3 and [next(w for w in ("vechat_amd.scrub", "vechat_amd.overlap", "vechat_amd.polish") if w in c) for c in log] == \
        ["vechat_amd.scrub", "vechat_amd.overlap", "vechat_amd.polish"]
    assert not any("minimap2" in c or c.startswith("yacrd") for c in log)
    scrubbed = (work / "reads.scrubbed.fq").read_text().split("\n")
    kept = {scrubbed[i][1:]: scrubbed[i + 1] for i in range(0, len(scrubbed) - 1, 4)}
    assert len(kept) >= 8 and all(h.startswith("@") for h in scrubbed[0:-1:4])
    by_name = {n: s.decode() for n, s in recs}
    for head, seq in kept.items():                           # a whole read under its name, or <name>_<begin>_<end>: the bases say which
        if head in by_name:
            assert seq == by_name[head]
        else:
            name, b, e = head.rsplit("_", 2)
            assert seq == by_name[name][int(b):int(e)]
    assert (work / "report.yacrd").exists()
    lines = out.read_text().split("\n")
    got = {lines[i][1:].split()[0]: lines[i + 1] for i in range(0, len(lines) - 1, 2)}
    assert got and all(lines[i].startswith(">") for i in range(0, len(lines) - 1, 2))
    assert {n.rstrip("r") for n in got} <= set(kept) and all(len(s) > 0 and set(s) <= set("ACGT") for s in got.values())
    assert len(got) >= len(kept) // 2
