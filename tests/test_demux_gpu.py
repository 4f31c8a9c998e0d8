"""The demultiplexer on the device, pinned to the CPU restatement of its rule (tests/demux_ref.py) array for array -- the views'
best hits, classes, labels, strands, ranges, the cut bytes, the groups and, where asked for, every hit: the hand-built cases of
tests/demux_cases.py, a seeded sweep over pattern counts, windows, flags and trim modes, the same call cut into 1, 2 and many
pieces of the budget, many calls in one process, the command line on simulated barcoded reads, and --consensus on three amplicons."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import demux_cases as DC
import demux_ref as R
import test_demux as TD
from vechat_amd import capi, demux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
BYTES = ("pc_bases", "pc_quals")
HITS = ("all_dist", "all_end")


def run_device(c, **more):
    return demux.demux_reads(c["reads"], c["patterns"], c["labels"], c["sides"], quals=c["quals"], **dict(c["params"], **more))


def differences(got, want):
    why = [f for f in TD.FIELDS if got[f].dtype != want[f].dtype or not np.array_equal(got[f], want[f])]
    why += [f for f in BYTES if got[f] != want[f]]
    why += [f for f in HITS if (got[f] is None) != (want[f] is None) or (want[f] is not None and (got[f].dtype != want[f].dtype or not np.array_equal(got[f], want[f])))]
    return why


def same(got, want):
    assert not differences(got, want), [(f, got[f][:8], want[f][:8]) for f in differences(got, want)]


def logged(capfd):
    return [tuple(int(x) for x in m) for m in re.findall(r"vc_demux: reads=(\d+) triples=(\d+) pieces=(\d+) accepted=(\d+)", capfd.readouterr().err)]


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_cases_equal_the_restatement(built, name, monkeypatch, capfd):
    c, want = DC.CASES[name], TD.restated(name)
    monkeypatch.setenv("VC_DEMUX_LOG", "1")
    got = run_device(c)
    same(got, want)
    TD.check_expect(c, got)
    n, P = len(c["reads"]), len(c["patterns"])
    (lr, lt, lp, la), = logged(capfd)
    assert (lr, lt, lp) == (n, 2 * n * P, 1) and got["stats"] == dict(reads=n, triples=2 * n * P, pieces=1, accepted=la)
    # every hit, whether or not the case asks for it: the search itself, triple by triple
    every = R.demux(c["reads"], c["patterns"], c["labels"], c["sides"], c["quals"], **dict(c["params"], flags=c["params"].get("flags", 0) | R.ALL_HITS))
    got = run_device(c, flags=c["params"].get("flags", 0) | R.ALL_HITS)
    same(got, every)
    permille = c["params"].get("max_err_permille", 200)
    assert la == sum(1 for i, d in enumerate(every["all_dist"]) if 1000 * int(d) <= permille * len(c["patterns"][i % P]))


@pytest.mark.parametrize("part", range(3))
def test_seeded_sweep_equals_the_restatement(built, part):
    """20 configurations from one seed (demux_cases.sweep; tests/test_demux.py holds them to every class and parameter value), seven a
    part.  Every mismatch of a part is reported, not the first."""
    cs, res = DC.sweep(), TD.restated_sweep()
    bad = []
    for i in range(7 * part, min(7 * part + 7, len(cs))):
        why = differences(run_device(cs[i]), res[i])
        if why:
            bad.append((i, cs[i]["params"], len(cs[i]["patterns"]), why))
    assert not bad, bad


def test_budget_pieces_give_identical_arrays(built, monkeypatch, capfd):
    """patterns_65 is 9 reads x 2 views x 65 patterns = 1170 results of 4 bytes: a budget of 1 MiB takes them at once, one of 2 400
    bytes four reads at a time and the last one alone, one of 2 700 bytes five and four, one of 600 bytes (and one of 1 byte) a read
    at a time"""
    c, want = DC.CASES["patterns_65"], TD.restated("patterns_65")
    monkeypatch.setenv("VC_DEMUX_LOG", "1")
    for mib, pieces in (("1", 1), (str(2400 / 1048576), 3), (str(2700 / 1048576), 2), (str(600 / 1048576), 9), (str(1 / 1048576), 9)):
        monkeypatch.setenv("VC_DEMUX_BUDGET_MB", mib)
        got = run_device(c)
        same(got, want)
        (_, lt, lp, _), = logged(capfd)
        assert (lt, lp) == (1170, pieces) and got["stats"]["pieces"] == pieces, (mib, lp)


def test_many_calls_in_one_process(built):
    """The library keeps one set of result arrays a process: sizes that grow and shrink, an empty set, a call after
    vc_demux_release() -- each equal to the restatement, the first and the last to each other."""
    names = ("patterns_65", "length_0_and_1", "plus_and_minus_evidence", "patterns_1", "flip_with_qualities", "window_1", "patterns_65")
    first = None
    for i, name in enumerate(names):
        if i == len(names) - 1:
            demux.declare(capi.load_hip()).vc_demux_release()
        got = run_device(DC.CASES[name])
        same(got, TD.restated(name))
        first = first or got
        if i == 3:                                           # no read at all, between two calls that have some
            empty = demux.demux_reads([], [DC.B1, DC.B2], labels=[4, 2])
            assert all(len(empty[f]) == 0 for f in TD.FIELDS[:10]) and empty["piece_off"].tolist() == [0] and empty["grp_off"].tolist() == [0] * 6
            assert demux.demux_reads([], [])["grp_off"].tolist() == [0]
    same(got, first)
    with pytest.raises(RuntimeError, match="IUPAC"):
        demux.demux_reads([b"ACGT"], [b"ACXT"])


# ------------------------------------------------------------------------------------------------- the command line
def write_fastq(path, names, reads, quals):
    with open(path, "w") as f:
        for n, r, q in zip(names, reads, quals):
            f.write(f"@{n}\n{r.decode()}\n+\n{q.decode()}\n")


def test_command_line_on_the_recall_set(built, tmp_path):
    """`python -m vechat_amd.demux` as a process of its own on the 400 barcoded reads of tests/test_demux.py: the per-label files, the
    unassigned file and the report are, byte for byte, what the restatement predicts"""
    barcodes, reads, _ = TD.barcoded()
    names = [f"read{i}" for i in range(len(reads))]
    quals = [bytes(40 + (i + j) % 40 for j in range(len(r))) for i, r in enumerate(reads)]
    write_fastq(tmp_path / "reads.fastq", names, reads, quals)
    label_names = [f"bc{j:02d}" for j in range(len(barcodes))]
    (tmp_path / "barcodes.fa").write_text("".join(f">{n}\n{b.decode()}\n" for n, b in zip(label_names, barcodes)))
    want = R.demux(reads, barcodes, quals=quals)
    assert np.array_equal(want["label"], TD.recall_result()["label"])
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    p = subprocess.run([sys.executable, "-m", "vechat_amd.demux", "--report", "report.tsv", "--out-dir", "out", "--unassigned", "un.fastq", "barcodes.fa", "reads.fastq"],
                       cwd=tmp_path, env=env, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    assert (tmp_path / "report.tsv").read_text() == R.format_report(names, label_names, label_names, want)
    pieces = R.pieces_of(want)
    record = lambda r: f"@{names[r]}\n{pieces[r][0].decode()}\n+\n{pieces[r][1].decode()}\n" if pieces[r][0] else ""
    for g, name in enumerate(label_names):
        assert (tmp_path / "out" / f"{name}.fastq").read_text() == "".join(record(r) for r in range(len(reads)) if want["label"][r] == g), name
    assert (tmp_path / "un.fastq").read_text() == "".join(record(r) for r in range(len(reads)) if want["label"][r] == R.UNASSIGNED)


FWD = [b"ACGGTCAGTTCGAGCATTCA", b"TGCAAGCTTGGATCCATGAC", b"GTTCAGGACCTAGRTACGAT"]
REV = [b"CCATGTTGACGGATAGCTAA", b"AGGCTTACCGATTGACTGCA", b"TCAGCGTTAACCGGATATCG"]


def amplicon_reads():
    """(the three amplicons, names, reads): ten reads an amplicon, each with ten substitutions inside the amplicon and one inside
    each primer, every other batch of three reverse-complemented.  The primers' outermost and innermost bases are left alone: an
    error on the last base of a primer makes the hit one base shorter (the smaller end wins), which is the rule and not the
    subject here."""
    rng = np.random.default_rng(21)
    inner = [DC.random_bases(rng, 300) for _ in range(3)]
    names, reads = [], []
    for k in range(30):
        a = k % 3
        body = bytearray(FWD[a].replace(b"R", b"G") + inner[a] + DC.rc(REV[a]))
        for x in [5, len(body) - 6] + [int(x) for x in rng.choice(np.arange(20, 320), 10, replace=False)]:
            body[x] = b"ACGT"[(b"ACGT".index(body[x]) + 1 + int(rng.integers(3))) % 4]
        reads.append(DC.rc(body) if (k // 3) % 2 else bytes(body))
        names.append(f"r{k}")
    return inner, names, reads


def test_consensus_of_three_amplicons_from_both_strands(built, tmp_path):
    """three amplicons of 300 bases between a forward and a reverse primer each (one with a degenerate base), ten reads an amplicon
    with substitutions, half of them reverse-complemented: `--orient --consensus` returns each amplicon without its primers, in
    the forward orientation"""
    fwd, rev = FWD, REV
    inner, names, reads = amplicon_reads()
    (tmp_path / "reads.fasta").write_text("".join(f">{n}\n{r.decode()}\n" for n, r in zip(names, reads)))
    (tmp_path / "primers.fa").write_text("".join(f">amp{a}:head\n{fwd[a].decode()}\n>amp{a}:tail\n{rev[a].decode()}\n" for a in range(3)))
    assert demux.main(["--orient", "--consensus", str(tmp_path / "out.fa"), str(tmp_path / "primers.fa"), str(tmp_path / "reads.fasta")]) == 0
    lines = (tmp_path / "out.fa").read_text().split("\n")
    assert lines[0::2] == [">amp0 size=10", ">amp1 size=10", ">amp2 size=10", ""]
    assert [s.encode() for s in lines[1::2]] == inner
