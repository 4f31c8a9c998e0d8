"""The clusterer without a device: the CPU restatement of its rule (tests/cluster_ref.py) on the hand-built cases, the C ABI's
argument checks (which come before the device is touched), groups_of, the TSV and FASTA texts, the command line's arguments, and
what the rule finds on simulated reads of two loci through the two restatements.  The device itself is pinned to the restatement
in tests/test_cluster_gpu.py."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import cluster_cases as CC
import cluster_ref as R
import overlap_ref as OR
from test_driver import simulate
from vechat_amd import capi, cluster

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ARRAYS = ("cl_off", "members", "cl_root", "cl_twisted", "cluster", "strand")


def invariants(c, res):
    """what holds for every answer, whatever the case"""
    n, k = len(c["lengths"]), len(res["cl_root"])
    off = [int(x) for x in res["cl_off"]]
    assert len(off) == k + 1 and off[0] == 0 and off[-1] == len(res["members"]) and len(res["cluster"]) == len(res["strand"]) == n
    assert len(set(res["members"].tolist())) == len(res["members"])
    P = dict(R.DEFAULTS, **c["params"])
    for j in range(k):
        rows = res["members"][off[j]:off[j + 1]].tolist()
        assert len(rows) >= P["min_size"] and min(rows) == int(res["cl_root"][j]) and all(int(res["cluster"][r]) == j for r in rows)
        assert res["strand"][int(res["cl_root"][j])] == 0
        key = (lambda r: (-c["lengths"][r], r)) if P["longest_first"] else (lambda r: r)
        assert rows == sorted(rows, key=key)
        if res["cl_twisted"][j]:
            assert not any(res["strand"][r] for r in rows)
    sizes = np.diff(np.array(off))
    order = [(-int(s), int(r)) for s, r in zip(sizes, res["cl_root"])] if P["by_size"] else [int(r) for r in res["cl_root"]]
    assert order == sorted(order)
    assert int((res["cluster"] != R.NONE).sum()) == len(res["members"])
    assert res["stats"]["kept"] == k <= res["stats"]["components"] <= n and res["stats"]["records"] == len(c["records"])


# ---------------------------------------------------------------------------------------------------- restatement
@functools.lru_cache(maxsize=None)
def restated(name):
    c = CC.CASES[name]
    return R.cluster(c["lengths"], c["records"], **c["params"])


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_restatement_on_the_case_table(name):
    c, res = CC.CASES[name], restated(name)
    invariants(c, res)
    x = c["expect"]
    for f in ARRAYS:
        assert res[f].tolist() == x[f], f
    assert (res["stats"]["links"], res["stats"]["components"], res["stats"]["kept"]) == (x["links"], x["components"], x["kept"])


def test_record_order_does_not_matter_to_the_restatement():
    for name in sorted(CC.CASES):
        c, want = CC.CASES[name], restated(name)
        order = np.random.default_rng(4).permutation(len(c["records"]))
        for recs in (c["records"][::-1], [c["records"][i] for i in order]):
            got = R.cluster(c["lengths"], recs, **c["params"])
            for f in ARRAYS:
                assert np.array_equal(got[f], want[f]), (name, f)


def test_the_large_cases_are_what_they_say():
    c = CC.CASES["path_of_300_reads_with_scrambled_ids"]
    assert len(c["lengths"]) == 300 and len(c["records"]) == 299 and restated("path_of_300_reads_with_scrambled_ids")["depth"] >= 150
    assert 0 < sum(c["expect"]["strand"]) < 300
    c = CC.CASES["star_with_a_hub_of_degree_500"]
    ends = [r[0] for r in c["records"]] + [r[1] for r in c["records"]]
    assert ends.count(500) == 500 and max(ends) == 500 and c["expect"]["cl_root"] == [0] and 0 < sum(c["expect"]["strand"]) < 501
    c = CC.CASES["path_and_star_side_by_side"]
    assert c["expect"]["cl_root"] == [0, 301] and c["expect"]["cl_off"] == [0, 300, 801] and c["expect"]["cluster"][300] == CC.N
    firsts = [r[0] < 300 for r in c["records"]]
    assert firsts != sorted(firsts) and firsts != sorted(firsts, reverse=True)          # the two components' records are mixed


@functools.lru_cache(maxsize=None)
def restated_sweep():
    return tuple(R.cluster(c["lengths"], c["records"], **c["params"]) for c in CC.sweep())


def test_sweep_configurations_cover_the_parameters():
    cs, res = CC.sweep(), restated_sweep()
    assert len(cs) == 36 and max(len(c["lengths"]) for c in cs) > 1500 and max(len(c["records"]) for c in cs) > 4000
    for f, vals in (("min_overlap", {0, 300, 500, 1000}), ("min_cover_permille", {0, 500, 800, 1000}), ("cover_both", {0, 1}),
                    ("min_identity_permille", {0, 800, 950}), ("min_size", {1, 2, 3, 10}), ("by_size", {0, 1}), ("longest_first", {0, 1})):
        assert {c["params"][f] for c in cs} == vals, f
    for c, r in zip(cs, res):
        invariants(c, r)
    assert sum(int(r["cl_twisted"].sum()) for r in res) >= 5 and sum(1 for r in res if len(r["cl_twisted"]) and not r["cl_twisted"].all()) >= 10
    assert sum(1 for r in res if (r["cluster"] == R.NONE).any()) >= 10 and sum(1 for r in res if len(r["cl_root"]) >= 2) >= 10
    assert max(r["depth"] for r in res) > 64 and sum(1 for r in res if r["strand"].any()) >= 10
    assert any(r["stats"]["links"] == 0 for r in res) and any(0 < r["stats"]["links"] < r["stats"]["records"] for r in res)


# ------------------------------------------------------------------------------------------- two loci, simulated reads
SIM = dict(n_reads=12, genome_len=1500, read_len=1500, err=0.06)
SEEDS = (5, 6)


@functools.lru_cache(maxsize=None)
def two_loci():
    """12 amplicon reads of 1.5 kb from each of two unrelated random loci (tests/test_driver.py's simulate: two haplotypes, both
    strands, 6 % errors), interleaved: (names, reads, locus per read, '+' / '-' per read)"""
    sets = []
    with tempfile.TemporaryDirectory() as d:
        for seed in SEEDS:
            sets.append(simulate(os.path.join(d, "sim.fq"), seed=seed, **SIM)[0])
    names, reads, locus, sign = [], [], [], []
    for i in range(SIM["n_reads"]):
        for x, recs in enumerate(sets):
            names.append("AB"[x] + recs[i][0])
            reads.append(recs[i][1])
            locus.append(x)
            sign.append(recs[i][0][-1])
    return tuple(names), tuple(reads), tuple(locus), tuple(sign)


def truth_of(locus, sign):
    """(cluster, strand) per read when the clusters are the loci, numbered by their first read"""
    first = {x: locus.index(x) for x in sorted(set(locus))}
    return [sorted(first).index(x) for x in locus], [int(sign[r] != sign[first[x]]) for r, x in enumerate(locus)]


@functools.lru_cache(maxsize=None)
def two_loci_restated():
    _, reads, _, _ = two_loci()
    ov = OR.overlaps(list(reads), None)
    return ov, R.cluster([len(s) for s in reads], R.rows_of(ov))


def test_two_simulated_loci_through_the_two_restatements():
    """The rule itself, on the CPU, through the overlapper's restatement (drop_internal 1) and the clusterer's, at the defaults of
    both: exactly two clusters, every read in the cluster of its locus, every strand as simulated.  profiles/cluster_recall.txt
    records the counts."""
    names, reads, locus, sign = two_loci()
    ov, res = two_loci_restated()
    want_cluster, want_strand = truth_of(locus, sign)
    cross = sum(1 for r in ov if locus[int(r["q_id"])] != locus[int(r["t_id"])])
    print(f"{len(reads)} reads of {SIM['read_len']} bp from 2 loci, {SIM['err']:.0%} errors, seeds {SEEDS}: {len(ov)} records ({cross} between the loci), "
          f"{res['stats']['links']} links, {res['stats']['components']} components, {res['stats']['kept']} kept, sizes "
          f"{np.diff(res['cl_off'].astype(np.int64)).tolist()}, twisted {res['cl_twisted'].tolist()}, reads on the reverse strand "
          f"{int(res['strand'].sum())}, reads placed as simulated {sum(int(a == b) for a, b in zip(res['cluster'].tolist(), want_cluster))}, "
          f"strands as simulated {sum(int(a == b) for a, b in zip(res['strand'].tolist(), want_strand))}")
    assert set(sign) == {"+", "-"} and len(reads) == 24
    assert res["stats"]["kept"] == 2 and res["cl_twisted"].tolist() == [0, 0]
    assert res["cluster"].tolist() == want_cluster
    assert res["strand"].tolist() == want_strand
    groups = R.groups_of(res, reads)
    assert [len(g) for g in groups] == [12, 12] and groups[0][0] == reads[0] and groups[1][0] == reads[1]


# ------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib(built):
    return capi.load_hip()


def test_header_exports_exist(lib):
    for sym in ("vc_cluster", "vc_cluster_default_params", "vc_cluster_last_error", "vc_cluster_release"):
        assert hasattr(lib, sym), sym
    p = cluster.default_params(lib)
    assert [p.device] + [getattr(p, f) for f in cluster.PARAMS] == [0, 500, 800, 1, 0, 2, 0, 0]
    assert {f: getattr(p, f) for f in cluster.PARAMS} == R.DEFAULTS
    header = " ".join(open(os.path.join(ROOT, "include", "vechat_hip.h")).read().split())
    for word in ("vc_cluster_params", "vc_cluster_in", "vc_cluster_out", "THIS IS THE LIBRARY'S OWN RULE: single-linkage clustering on qualified overlaps",
                 "It restates no other tool", "VC_CLUSTER_NONE 0xFFFFFFFFu", "1000 * matches >= min_identity_permille * block",
                 "ca = 1000 * (q_end - q_begin) >= min_cover_permille * len[a]", "joins (2 a, 2 b + g) and (2 a + 1, 2 b + 1 - g)",
                 "root[r] = label(2 r) >> 1", "strand[r] = label(2 r) & 1", "twisted[r] = label(2 r) == label(2 r + 1)", "Equality passes every threshold",
                 "by size descending, ties by root ascending", "by len descending, ties by index ascending",
                 "vc_cluster: records=M links=L rounds=R components=C kept=K"):
        assert word in header, word
    assert cluster.NONE == R.NONE == CC.N == 0xFFFFFFFF
    assert tuple(f for f, _ in cluster.RECORD_FIELDS) == R.FIELDS == CC.FIELDS


NO_DEVICE = 9999       # an ordinal no machine has: what passes the argument checks ends as VC_ERR_NO_DEVICE, with or without a GPU


def test_arguments_are_checked_before_the_device_in_the_documented_order(lib):
    cluster.declare(lib)
    u32 = lambda v: np.array(v, np.uint32)
    good = dict(len=u32([100, 50]), q_id=u32([0, 1]), t_id=u32([1, 0]), strand=np.array([0, 1], np.uint8), q_begin=u32([0, 10]), q_end=u32([100, 50]),
                t_begin=u32([5, 0]), t_end=u32([50, 100]), matches=u32([90, 80]), block=u32([100, 100]))
    kinds = dict(cluster.RECORD_FIELDS, len=C.c_uint32)
    out = cluster.VcClusterOut()

    def call(n=2, m=2, params=None, **replace):
        """one call with the good arrays, some replaced (None: a NULL pointer)"""
        use = dict(good, **replace)
        ptr = {k: (use[k].ctypes.data_as(C.POINTER(kinds[k])) if use[k] is not None else None) for k in kinds}
        a = cluster.VcClusterIn(n, ptr["len"], m, *[ptr[f] for f, _ in cluster.RECORD_FIELDS])
        p = cluster.default_params(lib, device=NO_DEVICE, **(params or {}))
        rc = lib.vc_cluster(C.byref(p), C.byref(a), C.byref(out))
        assert not out.cl_off and not out.members and not out.cluster and not out.strand and out.n_clusters == 0     # a failed call leaves every pointer NULL
        return rc, lib.vc_cluster_last_error().decode()

    assert call()[0] == capi.VC_ERR_NO_DEVICE                    # everything in order: only the device is missing
    assert call(n=0, m=0)[0] == capi.VC_ERR_NO_DEVICE
    assert call(m=0, **{f: None for f, _ in cluster.RECORD_FIELDS})[0] == capi.VC_ERR_NO_DEVICE
    assert call(t_id=u32([0, 1]), t_end=u32([50, 50]), strand=np.array([1, 1], np.uint8))[0] == capi.VC_ERR_NO_DEVICE      # a read with itself is legal
    for kw in (dict(min_overlap=0), dict(min_cover_permille=0), dict(min_cover_permille=1000), dict(min_identity_permille=1000), dict(min_size=1 << 30)):
        assert call(params=kw)[0] == capi.VC_ERR_NO_DEVICE, kw
    p = cluster.default_params(lib, device=NO_DEVICE)
    a = cluster.VcClusterIn()
    assert lib.vc_cluster(None, C.byref(a), C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_cluster(C.byref(p), None, C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_cluster(C.byref(p), C.byref(a), None) == capi.VC_ERR_ARG
    # one condition at a time, each VC_ERR_ARG
    long_read = dict(len=u32([100, (1 << 30) + 1]))
    one = [dict(len=None)] + [{f: None} for f, _ in cluster.RECORD_FIELDS]
    one += [dict(params=kw) for kw in (dict(min_overlap=-1), dict(min_cover_permille=-1), dict(min_cover_permille=1001), dict(cover_both=2), dict(cover_both=-1),
                                        dict(min_identity_permille=-1), dict(min_identity_permille=1001), dict(min_size=0), dict(by_size=2),
                                        dict(longest_first=2), dict(longest_first=-1))]
    one += [dict(q_id=u32([0, 2])), dict(t_id=u32([2, 0])), dict(q_begin=u32([100, 10])), dict(t_begin=u32([5, 100])), dict(q_end=u32([101, 50])),
            dict(t_end=u32([51, 100])), dict(strand=np.array([0, 2], np.uint8)), long_read, dict(n=(1 << 30) + 1)]      # the read count is refused before a length is read
    for kw in one:
        rc, msg = call(**kw)
        assert rc == capi.VC_ERR_ARG and msg, kw
    # the order: NULL pointers, parameters, records, the envelope -- the earlier one is the one reported
    order = [(dict(t_id=None), "NULL"), (dict(params=dict(min_size=0)), "min_size"), (dict(q_end=u32([101, 50])), "outside its read"), (long_read, "envelope")]
    for i, (kw, word) in enumerate(order):
        assert word in call(**kw)[1], (kw, word)
        for later, _ in order[i + 1:]:
            assert word in call(**dict(later, **kw))[1], (kw, later)
    # within the parameters and within a record: the order of the header
    assert "min_overlap" in call(params=dict(min_overlap=-1, min_cover_permille=2000, cover_both=3, min_size=0))[1]
    assert "min_cover_permille" in call(params=dict(min_cover_permille=2000, cover_both=3, min_identity_permille=-5))[1]
    assert "cover_both" in call(params=dict(cover_both=3, min_identity_permille=-5, by_size=7))[1]
    assert "min_identity_permille" in call(params=dict(min_identity_permille=-5, min_size=0))[1]
    assert "by_size" in call(params=dict(by_size=7, longest_first=7))[1]
    assert "not there" in call(q_id=u32([0, 7]), q_begin=u32([0, 60]))[1]
    assert "empty" in call(q_begin=u32([0, 50]), t_end=u32([50, 101]))[1]
    assert "outside its read" in call(t_end=u32([50, 101]), strand=np.array([0, 5], np.uint8))[1]
    assert "strand" in call(strand=np.array([0, 5], np.uint8), **long_read)[1]
    assert "VC_CLUSTER_MAX_READS" in call(n=(1 << 30) + 1)[1] and "VC_OVL_MAX_LEN" in call(m=0, len=u32([100, 1 << 31]))[1]
    lib.vc_cluster_release()


def test_python_run_refuses_what_does_not_fit(lib):
    with pytest.raises(TypeError):
        cluster.default_params(lib, no_such_field=1)
    recs = CC.columns([CC.rec([10, 10], 0, 1)])
    with pytest.raises(ValueError, match="does not fit"):
        cluster.run([10, 10], dict(recs, strand=np.array([256])), lib=lib, device=NO_DEVICE)
    with pytest.raises(ValueError, match="different lengths"):
        cluster.run([10, 10], dict(recs, block=np.array([5, 5])), lib=lib, device=NO_DEVICE)
    with pytest.raises(RuntimeError, match="not there"):
        cluster.run([10], recs, lib=lib, device=NO_DEVICE)


# ------------------------------------------------------------------------------------- groups, texts and arguments
HAND = dict(cl_off=np.array([0, 3, 5], np.uint64), members=np.array([3, 1, 4, 0, 5], np.uint32), cl_root=np.array([1, 0], np.uint32),
            cl_twisted=np.array([0, 1], np.uint8), cluster=np.array([1, 0, 0xFFFFFFFF, 0, 0, 1], np.uint32), strand=np.array([0, 0, 1, 1, 0, 0], np.uint8))
HAND_READS = [b"AACC", b"ACGTT", b"GGGA", b"AAACg", b"TTTT", b"CATN"]
HAND_NAMES = ["r0", "r1", "r2", "r3", "r4", "r5"]


def test_groups_of_orients_members_and_keeps_their_order():
    want = [[b"cGTTT", b"ACGTT", b"TTTT"], [b"AACC", b"CATN"]]          # r3 reverse-complemented, lower case kept; N stays N
    assert cluster.groups_of(HAND, HAND_READS) == want == R.groups_of(HAND, HAND_READS)
    assert cluster.groups_of(HAND, [bytearray(s) for s in HAND_READS]) == want
    empty = dict(HAND, cl_off=np.array([0], np.uint64), members=np.zeros(0, np.uint32))
    assert cluster.groups_of(empty, HAND_READS) == []


def test_tsv_and_consensus_texts():
    tsv = "r0\t1\t?\nr1\t0\t+\nr2\t*\t-\nr3\t0\t-\nr4\t0\t+\nr5\t1\t?\n"
    assert cluster.format_tsv(HAND_NAMES, HAND) == tsv == R.format_tsv(HAND_NAMES, HAND)
    assert cluster.format_consensus(HAND_NAMES, HAND, [b"ACGTT", b"AACC"]) == ">cluster_0 size=3 root=r1\nACGTT\n>cluster_1 size=2 root=r0\nAACC\n"
    assert cluster.format_consensus(HAND_NAMES, dict(HAND, cl_off=np.array([0], np.uint64)), []) == ""


def test_records_from_a_paf_file(tmp_path):
    (tmp_path / "o.paf").write_text("r1\t100\t5\t95\t-\tr0\t120\t10\t110\t80\t100\t255\tcg:Z:90M\n\nr0\t120\t0\t50\t+\tr2\t60\t10\t60\t45\t50\t255\n")
    rec = cluster.records_from_paf(str(tmp_path / "o.paf"), ["r0", "r1", "r2"])
    assert [tuple(int(rec[f][i]) for f in CC.FIELDS) for i in range(2)] == [(1, 0, 1, 5, 95, 10, 110, 80, 100), (0, 2, 0, 0, 50, 10, 60, 45, 50)]
    with pytest.raises(ValueError, match="not a read"):
        cluster.records_from_paf(str(tmp_path / "o.paf"), ["r0", "r1"])


def test_command_line_arguments(capsys):
    a = cluster.parse_args(["reads.fq"])
    assert (a.preset, a.paf, a.tsv, a.consensus, a.algorithm, a.min_identity, a.device, a.reads) == ("ava-ont", None, None, None, 1, None, 0, "reads.fq")
    assert a.params == {f: v for f, v in R.DEFAULTS.items() if f != "min_identity_permille"}
    a = cluster.parse_args(["-x", "ava-pb", "--min-overlap", "300", "--min-cover", "0.5", "--either", "--min-identity", "0.9", "--min-size", "3", "--by-size",
                            "--longest-first", "--paf", "o.paf", "--tsv", "c.tsv", "--consensus", "c.fa", "-l", "2", "--device", "1", "reads.fq"])
    assert a.params == dict(min_overlap=300, min_cover_permille=500, cover_both=0, min_size=3, by_size=1, longest_first=1)
    assert (a.preset, a.paf, a.tsv, a.consensus, a.algorithm, a.min_identity, a.device) == ("ava-pb", "o.paf", "c.tsv", "c.fa", 2, 0.9, 1)
    assert [cluster.parse_args(["--min-cover", f, "r"]).params["min_cover_permille"] for f in ("0", "0.0015", "0.3333", "0.29", "1")] == [0, 2, 333, 290, 1000]
    for bad in (["-x", "map-ont", "r"], ["--min-overlap", "-1", "r"], ["--min-cover", "1.5", "r"], ["--min-identity", "-0.1", "r"], ["--min-size", "0", "r"],
                ["-l", "3", "r"], []):
        with pytest.raises(SystemExit):
            cluster.parse_args(bad)
    with pytest.raises(SystemExit):
        cluster.parse_args(["--help"])
    assert "restates no other tool" in " ".join(capsys.readouterr().out.split())
