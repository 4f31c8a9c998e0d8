"""The clusterer on the device, pinned to the CPU restatement of its rule (tests/cluster_ref.py) array for array -- offsets, members,
roots, twists, the cluster and the strand of every read: the hand-built cases of tests/cluster_cases.py in the order given, reversed
and shuffled, a seeded sweep over all parameters, many calls in one process, cluster_reads on simulated reads of two loci, and the
command line with --tsv and --consensus."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as CC
import cluster_ref as R
import test_cluster as TC
from vechat_amd import capi, cluster, overlap, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
ARRAYS = TC.ARRAYS


def differing(got, want):
    return [f for f in ARRAYS if got[f].dtype != want[f].dtype or not np.array_equal(got[f], want[f])]


def same(got, want):
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (f, got[f][:8], want[f][:8])
    assert got["stats"] == dict(want["stats"], rounds=1 if want["stats"]["links"] else 0)


def logged(capfd):
    return [tuple(int(x) for x in m) for m in re.findall(r"vc_cluster: records=(\d+) links=(\d+) rounds=(\d+) components=(\d+) kept=(\d+)", capfd.readouterr().err)]


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_cases_equal_the_restatement(built, name, monkeypatch, capfd):
    c, want = CC.CASES[name], TC.restated(name)
    monkeypatch.setenv("VC_CLUSTER_LOG", "1")
    got = cluster.run(c["lengths"], CC.columns(c["records"]), **c["params"])
    same(got, want)
    x = c["expect"]
    for f in ARRAYS:
        assert got[f].tolist() == x[f], f
    assert logged(capfd) == [(len(c["records"]), x["links"], 1 if x["links"] else 0, x["components"], x["kept"])]
    # the records reversed and shuffled
    order = np.random.default_rng(4).permutation(len(c["records"]))
    same(cluster.run(c["lengths"], CC.columns(c["records"][::-1]), **c["params"]), want)
    same(cluster.run(c["lengths"], CC.columns([c["records"][i] for i in order]), **c["params"]), want)


@pytest.mark.parametrize("part", range(3))
def test_seeded_sweep_equals_the_restatement(built, part):
    """36 record sets from one seed (cluster_cases.sweep; tests/test_cluster.py holds them to twisted clusters, dropped reads, both
    values of every flag and a component deeper than 64), twelve a part.  Every mismatch of a part is reported, not the first."""
    cs, res = CC.sweep(), TC.restated_sweep()
    bad = []
    for i in range(12 * part, 12 * part + 12):
        c, want = cs[i], res[i]
        got = cluster.run(c["lengths"], CC.columns(c["records"]), **c["params"])
        why = differing(got, want) + [f for f in ("records", "links", "components", "kept") if got["stats"][f] != want["stats"][f]]
        if why:
            bad.append((i, c["params"], why))
    assert not bad, bad


def test_many_calls_in_one_process(built):
    """The library keeps one set of result arrays a process: sizes that grow and shrink, an empty set, a call after
    vc_cluster_release() -- each equal to the restatement, the first and the last to each other."""
    names = ("path_and_star_side_by_side", "one_pair", "star_with_a_hub_of_degree_500", "no_records", "path_of_300_reads_with_scrambled_ids",
             "twisted_triangle", "path_and_star_side_by_side")
    first = None
    for i, name in enumerate(names):
        c = CC.CASES[name]
        if i == len(names) - 1:
            cluster.declare(capi.load_hip()).vc_cluster_release()
        got = cluster.run(c["lengths"], CC.columns(c["records"]), **c["params"])
        same(got, TC.restated(name))
        first = first or got
        if i == 3:                                           # no read at all, between two calls that have some
            empty = cluster.run([], CC.columns([]))
            assert empty["cl_off"].tolist() == [0] and all(len(empty[f]) == 0 for f in ARRAYS if f != "cl_off")
            assert empty["stats"] == dict(records=0, links=0, rounds=0, components=0, kept=0)
    same(got, first)


def test_the_structured_array_of_the_overlapper_is_taken_as_it_is(built):
    c = CC.CASES["root_is_not_read_0"]
    recs = np.zeros(len(c["records"]), overlap.RECORD)
    for f, col in CC.columns(c["records"]).items():
        recs[f] = col
    same(cluster.run(c["lengths"], recs), TC.restated("root_is_not_read_0"))
    with pytest.raises(RuntimeError, match="outside its read"):
        cluster.run([10, 10], CC.columns([CC.rec([10, 11], 0, 1)]))


# ------------------------------------------------------------------------------------------- two loci, simulated reads
def test_cluster_reads_on_two_simulated_loci(built):
    """cluster_reads is find_overlaps plus vc_cluster: equal to the device's own records through the restatement, and -- the
    device overlapper being pinned to its restatement elsewhere -- to the two restatements and the simulated truth"""
    names, reads, locus, sign = TC.two_loci()
    got = cluster.cluster_reads(list(reads))
    ov = overlap.find_overlaps(list(reads), None, **overlap.PRESETS["ava-ont"])
    same(got, R.cluster([len(s) for s in reads], R.rows_of(ov)))
    same(got, TC.two_loci_restated()[1])
    want_cluster, want_strand = TC.truth_of(locus, sign)
    assert got["cluster"].tolist() == want_cluster and got["strand"].tolist() == want_strand
    # exact identities first: every record is aligned on the device, and nothing changes at 6 % errors and a floor of 80 %
    exact = cluster.cluster_reads(list(reads), min_identity=0.8, by_size=1, longest_first=1)
    ident = overlap.identity(ov, list(reads), None)
    same(exact, R.cluster([len(s) for s in reads], R.rows_of(ident), min_identity_permille=800, by_size=1, longest_first=1))
    assert sorted(exact["cl_root"].tolist()) == [0, 1]


def test_command_line_on_two_simulated_loci(built, tmp_path):
    """`python -m vechat_amd.cluster` as a process of its own on a FASTQ of the two loci: the TSV agrees with the simulated truth, and
    each consensus is byte for byte what poa.poa_consensus(cluster.groups_of(...)) returns in this process"""
    names, reads, locus, sign = TC.two_loci()
    with open(tmp_path / "reads.fq", "w") as fw:
        for n, s in zip(names, reads):
            fw.write(f"@{n}\n{s.decode()}\n+\n{'5' * len(s)}\n")
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    p = subprocess.run([sys.executable, "-m", "vechat_amd.cluster", "--longest-first", "--tsv", "out.tsv", "--consensus", "out.fa", "reads.fq"], cwd=tmp_path,
                       env=env, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    want_cluster, want_strand = TC.truth_of(locus, sign)
    tsv = "".join(f"{n}\t{c}\t{'+-'[s]}\n" for n, c, s in zip(names, want_cluster, want_strand))
    assert (tmp_path / "out.tsv").read_text() == tsv and p.stdout == b""
    res = cluster.cluster_reads(list(reads), longest_first=1)
    assert cluster.format_tsv(names, res) == tsv == R.format_tsv(names, res)
    groups = cluster.groups_of(res, reads)
    assert groups == R.groups_of(res, reads) and [len(g) for g in groups] == [12, 12]
    assert all(len(g[0]) == max(len(s) for s in g) for g in groups)          # the longest read is the backbone
    cons = poa.poa_consensus(groups)
    fasta = "".join(f">cluster_{c} size=12 root={names[c]}\n{cons[c].decode()}\n" for c in range(2))
    assert (tmp_path / "out.fa").read_text() == fasta
    assert all(len(s) > 1300 and set(s) <= set(b"ACGT") for s in cons)
