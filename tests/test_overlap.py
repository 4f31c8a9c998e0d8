"""The overlapper without a device: the CPU restatement of its rule on the hand-built cases and on simulated reads with known
origins, the C ABI's argument checks (which come before the device is touched), the PAF writer, the command line and the
driver's --overlapper device command lines.  The device itself is pinned to the restatement in tests/test_overlap_gpu.py."""
import ctypes as C
import functools
import io
import os
import re
import tempfile

import numpy as np
import pytest

import align_ref
import overlap_cases as OC
import overlap_ref as R
from test_driver import simulate
from vechat_amd import capi, driver, overlap

HERE = os.path.dirname(os.path.abspath(__file__))


def rows(recs):
    return [tuple(int(x) for x in r) for r in recs]


# ---------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", sorted(OC.SKETCH_CASES))
def test_restated_sketch_on_the_case_table(name):
    seqs, k, w, expect = OC.SKETCH_CASES[name]
    t = R.sketch(seqs, k, w)
    got = [(int(s), int(p)) for s, p in zip(t["seq"], t["pos"])]
    assert got == sorted(got) and len(set(got)) == len(got)
    for s, p in got:
        assert k - 1 <= p < len(seqs[s])
    if expect is not None:
        assert got == expect
    if name == "len_k_plus_w_minus_1":
        assert len(got) == 1
    if name == "homopolymer":
        assert len(set(int(h) for h in t["hash"])) == 1 and not t["strand"].any()        # AAAA.. is below TTTT..
    if name == "w_1_every_kmer":                                                         # every 4-mer but the palindromes
        assert len(got) == sum(1 for p in range(3, 60) if seqs[0][p - 3:p + 1] != OC.rc(seqs[0][p - 3:p + 1]))
    if name == "self_reverse_complement_kmer":
        assert all(not (s == 0 and p == 25) for s, p in got) and all(p not in (5, 11) for s, p in got if s == 1)   # GAATTC never


@pytest.mark.parametrize("name", sorted(OC.OVERLAP_CASES))
def test_restated_overlaps_on_the_case_table(name):
    c = OC.OVERLAP_CASES[name]
    r = R.overlaps(c["targets"], c["queries"], **c["params"])
    got = rows(r)
    record_invariants(got, c["targets"], c["queries"])
    if c["expect"] is not None:
        assert got == c["expect"]


def test_restated_records_of_whole_reads():
    """the answers a reader can check with the sequences in hand: an exact copy, a reverse-complemented piece, a contained piece"""
    c = OC.OVERLAP_CASES
    a = rows(R.overlaps(c["identical_sequences_same_set"]["targets"], None))
    assert [x[:3] for x in a] == [(0, 1, 0), (1, 0, 0)] and a[0][3:7] == a[1][3:7]
    q, t, st, qb, qe, tb, te = rows(R.overlaps(c["reverse_strand_touching_both_query_ends"]["targets"], c["reverse_strand_touching_both_query_ends"]["queries"]))[0][:7]
    assert st == 1 and qb <= 20 and qe >= 780 and abs((tb - 200) - (800 - qe)) <= 0 and abs((1000 - te) - qb) <= 0      # the same diagonal, reversed
    q, t, st, qb, qe, tb, te = rows(R.overlaps(c["containment_is_kept"]["targets"], c["containment_is_kept"]["queries"]))[0][:7]
    assert st == 0 and tb - qb == 300 and te - qe == 300
    for name in ("three_or_more_target_pieces", "default_budget"):
        assert len(R.overlaps(c[name]["targets"], None)) == 16


# --------------------------------------------------------------------------------------------------------- recall
@functools.lru_cache(maxsize=None)
def simulated(err, seed=11, **params):
    """60 reads of 3 kb from a 20 kb genome (two haplotypes), both strands: (sequences, (start, end, strand) per read, records of
    the restatement under `params`)"""
    with tempfile.TemporaryDirectory() as d:
        recs, _ = simulate(os.path.join(d, "sim.fq"), n_reads=60, genome_len=20000, read_len=3000, err=err, seed=seed)
    info = []
    for n, _ in recs:
        a = n.split("_")
        info.append((int(a[1]), int(a[2]), a[3]))
    seqs = tuple(s for _, s in recs)
    return seqs, tuple(info), R.overlaps(list(seqs), **params)


def recall(err, min_len, **params):
    seqs, info, ov = simulated(err, **params)
    got = {(int(r["q_id"]), int(r["t_id"])): r for r in ov}
    true = found = 0
    worst = 0
    for q in range(len(seqs)):
        for t in range(len(seqs)):
            lo, hi = max(info[q][0], info[t][0]), min(info[q][1], info[t][1])
            if q == t or hi - lo < min_len:
                continue
            true += 1
            r = got.get((q, t))
            if r is None or int(r["strand"]) != (info[q][2] != info[t][2]):
                continue
            found += 1
            # the truth, interpolated: genome interval [lo, hi) on each read, scaled to the read's own length, its strand applied
            for rid, b, e in ((q, int(r["q_begin"]), int(r["q_end"])), (t, int(r["t_begin"]), int(r["t_end"]))):
                s, en, st = info[rid]
                scale = len(seqs[rid]) / (en - s)
                tb, te = (lo - s) * scale, (hi - s) * scale
                if st == "-":
                    tb, te = len(seqs[rid]) - te, len(seqs[rid]) - tb
                worst = max(worst, abs(b - tb), abs(e - te))
    false = sum(1 for (q, t) in got if min(info[q][1], info[t][1]) <= max(info[q][0], info[t][0]))
    return found, true, false, worst


def test_recall_on_simulated_reads():
    """The rule itself, on the CPU: at 6 % errors every true overlap of >= 2000 bp is reported with the right strand and its ends
    within 100 bp of the interpolated truth, and no pair is reported whose reads do not overlap on the genome.
    (profiles/overlap_recall.txt records the counts, and the count at 10 % errors and >= 1000 bp, which is reported only.)"""
    found, true, false, worst = recall(0.06, 2000)
    print(f"6 % errors, >= 2000 bp: found {found} of {true}, false pairs {false}, worst end {worst:.1f} bp")
    assert true > 300
    assert found == true
    assert worst <= 100
    assert false == 0


def test_recall_on_simulated_reads_ava_pb():
    """The same four assertions at the product's default preset (ava-pb: k 19, w 5), on reads with 1 % errors: every true overlap of
    >= 2000 bp with the right strand and its ends within 100 bp of the interpolated truth, no false pair."""
    found, true, false, worst = recall(0.01, 2000, k=19, w=5)
    print(f"1 % errors, k 19 w 5, >= 2000 bp: found {found} of {true}, false pairs {false}, worst end {worst:.1f} bp, "
          f"{len(simulated(0.01, k=19, w=5)[2])} records")
    assert true > 300
    assert found == true
    assert worst <= 100
    assert false == 0


# ------------------------------------------------------------------------------- what the device tests are held to
# Shared with tests/test_overlap_gpu.py: each restatement is computed once a process.  The conditions that keep a device test from
# passing on an empty or one-sided answer are checked here, on the restatement, with no device.
CLASSES = ((4, 1), (4, 5), (16, 5), (17, 5), (19, 5), (19, 1), (28, 5), (28, 64), (15, 64))


@functools.lru_cache(maxsize=None)
def sixteen_reads():
    """16 reads of 1.2 kb with 2 % errors from a 4 kb genome, both strands"""
    with tempfile.TemporaryDirectory() as d:
        recs, _ = simulate(os.path.join(d, "sim.fq"), n_reads=16, genome_len=4000, read_len=1200, err=0.02, seed=5)
    return tuple(s for _, s in recs)


@functools.lru_cache(maxsize=None)
def restated_class(k, w):
    """the 16 reads against themselves at (k, w), min_overlap 300: (minimizer table, records, seeds by key)"""
    seqs = list(sixteen_reads())
    return R.sketch(seqs, k, w), R.overlaps(seqs, None, k=k, w=w, min_overlap=300), R.seeds(seqs, seqs, k, w, R.DEFAULTS["max_occ"], 1)


def class_preconditions(k, w):
    tab, recs, keys = restated_class(k, w)
    assert len(tab) and set(int(s) for s in recs["strand"]) == {0, 1}
    if k >= 17:
        assert int(tab["hash"].max()) >= 1 << 32
    if (k, w) == (4, 1):
        assert len(keys) >= 400 and len(recs) >= 1
    else:
        assert len(recs) >= 50
    return tab, recs, keys


@pytest.mark.parametrize("k,w", CLASSES)
def test_every_k_and_w_class_has_something_to_compare(k, w):
    tab, recs, keys = class_preconditions(k, w)
    print(f"k {k} w {w}: {len(tab)} minimizers, {len(recs)} records, {sum(len(a) for a in keys.values())} anchors in {len(keys)} keys")


@functools.lru_cache(maxsize=None)
def restated_repeats(max_occ):
    reads = OC.repeat_reads()
    return R.overlaps(reads, None, min_overlap=300, max_occ=max_occ), R.seeds(reads, reads, R.DEFAULTS["k"], R.DEFAULTS["w"], max_occ, 1)


def repeat_preconditions():
    (full, keys), (capped, _) = restated_repeats(R.DEFAULTS["max_occ"]), restated_repeats(20)
    assert max(len(a) for a in keys.values()) >= 1000
    assert len(full) and len(capped) and rows(full) != rows(capped)


def test_repeat_reads_fill_keys_and_max_occ_decides():
    repeat_preconditions()
    full, keys = restated_repeats(R.DEFAULTS["max_occ"])
    print(f"repeat reads: largest key {max(len(a) for a in keys.values())} anchors, {len(full)} records, {len(restated_repeats(20)[0])} with max_occ 20")


def _restate_config(c):
    P = dict(R.DEFAULTS, **c["params"])
    same = c["queries"] is None
    keys = R.seeds(c["targets"], c["targets"] if same else c["queries"], P["k"], P["w"], P["max_occ"], 1 if same else 0)
    tabs = [R.sketch(s, P["k"], P["w"]) for s in ((c["targets"],) if same else (c["targets"], c["queries"]))]
    return R.overlaps(c["targets"], c["queries"], **c["params"]), sum(len(a) for a in keys.values()), len(keys), tabs


@functools.lru_cache(maxsize=None)
def restated_sweep():
    """per configuration of overlap_cases.sweep(): (records, anchors, keys, [minimizer table of each set]); about a second in all"""
    return tuple(_restate_config(c) for c in OC.sweep())


def record_invariants(got, targets, queries):
    assert got == sorted(got, key=lambda x: x[:3])
    qs = targets if queries is None else queries
    for q, t, st, qb, qe, tb, te, n, score, matches, block in got:
        assert 0 <= qb < qe <= len(qs[q]) and 0 <= tb < te <= len(targets[t]) and block == max(qe - qb, te - tb) and matches <= block
        assert queries is not None or q != t


def test_sweep_configurations_give_records():
    """the 24 configurations of the seeded sweep: what they draw, the invariants of every record, and enough records that the device
    test compares something -- at least 16 configurations with a record and 200 records together"""
    cs, res = OC.sweep(), restated_sweep()
    assert len(cs) == len(res) == 24
    for c, (recs, _, _, _) in zip(cs, res):
        record_invariants(rows(recs), c["targets"], c["queries"])
        reads = c["targets"] + (c["queries"] or [])
        assert b"" in reads and any(0 < len(r) < c["params"]["k"] for r in reads) and all(len(r) <= 901 for r in reads)
    assert {c["budget_mb"] for c in cs} == {None, 0.01} and {c["queries"] is None for c in cs} == {False, True}
    assert any(r != r.upper() for c in cs for r in c["targets"]) and any(set(r) - set(b"ACGTacgt") for c in cs for r in c["targets"])
    counts = [len(recs) for recs, _, _, _ in res]
    print("records per configuration:", counts)
    assert sum(1 for n in counts if n) >= 16 and sum(counts) >= 200
    assert any(int(r["strand"]) for recs, _, _, _ in res for r in recs)


def test_twin_kmers_differ_above_bit_31_only():
    """what the case hashes_equal_in_their_low_32_bits stands on, checked with the restatement's own hash: two different 19-mers a pair,
    hashes equal below bit 32 and different above, and one minimizer entry for each k-mer of the four reads"""
    for (a, b, ha, hb), bit in zip(OC._tw, (32, 37)):
        assert a != b and len(a) == len(b) == 19
        got = [R.kmers(s, 19)[18] for s in (a, b)]
        assert [g[0] for g in got] == [ha, hb] and ha ^ hb == 1 << bit and ha & 0xFFFFFFFF == hb & 0xFFFFFFFF
        assert R.mix(OC.unmix(ha, 19), 19) == ha
    c = OC.OVERLAP_CASES["hashes_equal_in_their_low_32_bits"]
    assert [len(R.sketch([s], 19, 1)) for s in c["targets"] + c["queries"]] == [2, 2, 2, 2]
    keys = R.seeds(c["targets"], c["queries"], 19, 1, 100, 0)
    assert {k: len(a) for k, a in keys.items()} == {(0, 0, 0): 1, (1, 1, 0): 1}


def test_both_strands_of_one_pair():
    """target X + Y against query X + rc(Y): one pair, two keys, a record on each strand"""
    c = OC.OVERLAP_CASES["both_strands_of_one_pair"]
    got = rows(R.overlaps(c["targets"], c["queries"], **c["params"]))
    assert [x[:3] for x in got] == [(0, 0, 0), (0, 0, 1)]


# ---- the command line: two files, ava-pb
CLI_SEED = 7          # 11 and 12 PAF lines on both strands, 4 records dropped for their names
CLI_ARGS = (("-x", "ava-pb", "--min-overlap", "400", "--min-identity", "0.9", "targets.fa", "reads.fa"),
            ("-x", "ava-pb", "--min-overlap", "400", "targets.fa", "targets.fa"))
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@functools.lru_cache(maxsize=None)
def command_line_files(seed=None):
    """((name, sequence) of targets.fa, of reads.fa): six reads; reads 2..5 again under their own names and read 1 under a new one"""
    with tempfile.TemporaryDirectory() as d:
        recs, _ = simulate(os.path.join(d, "sim.fa"), n_reads=6, genome_len=1500, read_len=800, err=0.02, seed=CLI_SEED if seed is None else seed, fastq=False)
    return tuple(recs), tuple(recs[2:6]) + (("elsewhere", recs[1][1]),)


@functools.lru_cache(maxsize=None)
def command_line_expected(seed=None):
    """The PAF text of the two commands of CLI_ARGS, from the restatement and the aligner's CPU DP alone, and the number of records
    dropped for their names.  Nothing here calls into vechat_amd.overlap."""
    targets, reads = command_line_files(seed)
    texts, dropped = [], 0
    for queries, identity in ((reads, 0.9), (None, None)):
        qs = targets if queries is None else queries
        recs = rows(R.overlaps([s for _, s in targets], None if queries is None else [s for _, s in queries], k=19, w=5, min_overlap=400))
        kept = [r for r in recs if qs[r[0]][0] != targets[r[1]][0]]
        dropped += len(recs) - len(kept)
        lines = []
        for q, t, st, qb, qe, tb, te, _, _, matches, block in kept:
            if identity is not None:
                piece = qs[q][1][qb:qe]
                cigar, dist = align_ref.align(piece.translate(_COMP)[::-1] if st else piece, targets[t][1][tb:te])
                block = sum(int(x) for x in re.findall(r"(\d+)[MID]", cigar))
                matches = block - dist
                if not (float(matches) >= identity * float(block) and block >= 400):
                    continue
            lines.append("\t".join(str(x) for x in (qs[q][0], len(qs[q][1]), qb, qe, "-" if st else "+", targets[t][0], len(targets[t][1]), tb, te, matches, block, 255)) + "\n")
        texts.append("".join(lines))
    return tuple(texts), dropped


def command_line_preconditions():
    texts, dropped = command_line_expected()
    assert dropped >= 1
    for text in texts:
        lines = text.splitlines()
        assert len(lines) >= 4 and {l.split("\t")[4] for l in lines} == {"+", "-"}
    return texts


def test_command_line_case_has_lines_on_both_strands_and_a_name_to_drop():
    texts = command_line_preconditions()
    print(f"ava-pb command lines: {[len(t.splitlines()) for t in texts]} PAF lines expected, {command_line_expected()[1]} records dropped for their names")


# ------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib(built):
    return capi.load_hip()


def test_header_exports_exist(lib):
    for sym in ("vc_overlap", "vc_overlap_sketch", "vc_overlap_default_params", "vc_overlap_last_error", "vc_overlap_release"):
        assert hasattr(lib, sym), sym
    p = overlap.default_params(lib)
    assert [getattr(p, f) for f in overlap.PARAMS] == [15, 5, 100, 5000, 500, 64, 40, 3, 500, 1, 0]
    header = open(os.path.join(os.path.dirname(HERE), "include", "vechat_hip.h")).read()
    for word in ("vc_overlap_params", "VC_OVL_MAX_LEN", "x = (~x + (x << 21)) & mask", "NOT a\n * byte-for-byte restatement"):
        assert word in header, word


def _seqs(off, bases=b"ACGT" * 50):
    off = np.array(off, np.uint64)
    b = np.frombuffer(bases, np.uint8).copy()
    return overlap.VcOverlapSeqs(len(off) - 1, off.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_uint8))), (off, b)


NO_DEVICE = 9999       # an ordinal no machine has: what passes the argument checks ends as VC_ERR_NO_DEVICE, with or without a GPU


def test_arguments_are_checked_before_the_device_in_the_documented_order(lib):
    overlap.declare(lib)
    good, keep1 = _seqs([0, 100, 200])
    bad_start, keep2 = _seqs([1, 100, 200])
    bad_order, keep3 = _seqs([0, 150, 100])
    long_off = np.array([0, (1 << 30) + 1], np.uint64)           # checked on its length alone: the bases are never read
    long_one = overlap.VcOverlapSeqs(1, long_off.ctypes.data_as(C.POINTER(C.c_uint64)), keep1[1].ctypes.data_as(C.POINTER(C.c_uint8)))
    no_off = overlap.VcOverlapSeqs(2, None, keep1[1].ctypes.data_as(C.POINTER(C.c_uint8)))
    no_bases = overlap.VcOverlapSeqs(2, keep1[0].ctypes.data_as(C.POINTER(C.c_uint64)), None)
    out = overlap.VcOverlapOut()

    def call(t=good, q=good, **kw):
        p = overlap.default_params(lib, device=NO_DEVICE, **kw)
        rc = lib.vc_overlap(C.byref(p), C.byref(t) if t is not None else None, C.byref(q) if q is not None else None, C.byref(out))
        assert not out.q_id and out.n == 0                       # a failed call leaves every pointer NULL
        return rc, lib.vc_overlap_last_error().decode()

    assert call()[0] == capi.VC_ERR_NO_DEVICE                    # everything in order: only the device is missing
    assert call(q=None, same_set=1)[0] == capi.VC_ERR_NO_DEVICE  # same_set does not read the queries
    p = overlap.default_params(lib, device=NO_DEVICE)
    assert lib.vc_overlap(None, C.byref(good), C.byref(good), C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_overlap(C.byref(p), C.byref(good), C.byref(good), None) == capi.VC_ERR_ARG
    # one condition at a time, each VC_ERR_ARG
    for kw in (dict(t=None), dict(q=None), dict(t=no_off), dict(q=no_bases), dict(t=bad_start), dict(q=bad_order), dict(k=3), dict(k=29), dict(w=0),
               dict(w=65), dict(lookback=63), dict(lookback=65), dict(max_occ=0), dict(max_gap=-1), dict(bandwidth=0), dict(min_chain_score=0),
               dict(min_anchors=0), dict(min_overlap=-5), dict(drop_internal=2), dict(same_set=2), dict(max_occ=65537), dict(max_gap=(1 << 24) + 1),
               dict(bandwidth=(1 << 24) + 1), dict(t=long_one), dict(q=long_one)):
        rc, msg = call(**kw)
        assert rc == capi.VC_ERR_ARG and msg, kw
    # the order: NULL pointers, offsets, k, w, lookback and the limits, the envelope -- the earlier one is the one reported
    order = [(dict(t=None), "NULL"), (dict(t=bad_start), "start at 0"), (dict(k=3), "k outside"), (dict(w=0), "w outside"),
             (dict(lookback=1), "lookback"), (dict(max_gap=0), "zero or negative"), (dict(max_occ=65537), "envelope"), (dict(q=long_one), "envelope")]
    for i, (kw, word) in enumerate(order):
        assert word in call(**kw)[1], (kw, word)
        for later, _ in order[i + 1:]:
            if set(kw) & set(later):
                continue
            assert word in call(**dict(later, **kw))[1], (kw, later)
    # the sketch entry, same order
    so = overlap.VcOverlapSketchOut()
    assert lib.vc_overlap_sketch(NO_DEVICE, 15, 5, C.byref(good), C.byref(so)) == capi.VC_ERR_NO_DEVICE
    for args in ((15, 5, None), (15, 5, bad_start), (15, 5, bad_order), (3, 5, good), (29, 5, good), (15, 0, good), (15, 65, good), (15, 5, long_one)):
        assert lib.vc_overlap_sketch(NO_DEVICE, args[0], args[1], C.byref(args[2]) if args[2] is not None else None, C.byref(so)) == capi.VC_ERR_ARG, args[:2]
        assert not so.hash
    assert lib.vc_overlap_sketch(NO_DEVICE, 15, 5, C.byref(good), None) == capi.VC_ERR_ARG
    assert lib.vc_overlap_sketch(NO_DEVICE, 3, 5, C.byref(bad_start), C.byref(so)) == capi.VC_ERR_ARG
    assert "offsets" in lib.vc_overlap_last_error().decode()
    lib.vc_overlap_release()
    del keep2, keep3


# ------------------------------------------------------------------------------------------ PAF and the command line
def test_write_paf_and_the_command_line_arguments(tmp_path, capsys):
    recs = np.zeros(2, overlap.RECORD)
    recs[0] = (1, 0, 0, 5, 905, 100, 1000, 60, 850, 880, 900)
    recs[1] = (0, 1, 1, 0, 700, 20, 725, 40, 600, 650, 705)
    path = tmp_path / "o.paf"
    overlap.write_paf(str(path), recs, ["t0", "t1"], [1500, 800], ["q0", "q1"], [700, 1000])
    assert path.read_text() == "q1\t1000\t5\t905\t+\tt0\t1500\t100\t1000\t880\t900\t255\nq0\t700\t0\t700\t-\tt1\t800\t20\t725\t650\t705\t255\n"
    buf = io.StringIO()
    overlap.write_paf(buf, recs[:0], [], [], [], [])
    assert buf.getvalue() == ""
    assert overlap.RECORD == R.REC and overlap.SKETCH == R.TAB              # the two sides describe one layout, each in its own words
    a = overlap.parse_args(["t.fa", "r.fa"])
    assert (a.preset, a.min_overlap, a.min_identity, a.threads, a.targets, a.reads) == ("ava-ont", 500, None, 1, "t.fa", "r.fa")
    a = overlap.parse_args(["-x", "ava-pb", "--min-overlap", "1000", "--min-identity", "0.99", "--threads", "8", "t.fa", "r.fa"])
    assert (a.preset, a.min_overlap, a.min_identity, a.threads) == ("ava-pb", 1000, 0.99, 8)
    assert overlap.PRESETS["ava-pb"]["k"] == 19 and overlap.PRESETS["ava-ont"]["k"] == 15
    for bad in (["-x", "map-ont", "t", "r"], ["--min-overlap", "0", "t", "r"], ["--min-identity", "1.5", "t", "r"], ["t"]):
        with pytest.raises(SystemExit):
            overlap.parse_args(bad)
    capsys.readouterr()
    with pytest.raises(TypeError):
        overlap.default_params(None, no_such_field=1)


# -------------------------------------------------------------------------------------------------------- driver
def test_driver_overlapper_device_command_lines(tmp_path, monkeypatch):
    reads = tmp_path / "reads.fastq"
    simulate(str(reads), n_reads=4)
    cmds = []

    def fake_sh(cmd, cwd):                                     # no tool runs: every command's output file appears empty
        cmds.append(cmd)
        open(os.path.join(cwd, cmd.rsplit(">", 1)[1].strip().strip("'")), "w").close()

    monkeypatch.setattr(driver, "_sh", fake_sh)
    import shlex
    import sys
    py, rd = shlex.quote(sys.executable), shlex.quote(str(reads))

    def run(extra):
        del cmds[:]
        work = tmp_path / "work"
        assert driver.main([str(reads), "-o", str(tmp_path / "out.fa"), "--workdir", str(work), "--overlapper", "device", "--polisher", "POL"] + extra) == 0
        return [c for c in cmds if "vechat_amd.overlap" in c], shlex.quote(str(work / "overlap.paf")), shlex.quote(str(work / "reads.corrected.tmp1.fa"))

    ov, paf, r1 = run(["--platform", "ont", "-t", "4"])
    assert ov == [f"{py} -m vechat_amd.overlap -x ava-ont --threads 4 {rd} {rd} >{paf}",
                  f"{py} -m vechat_amd.overlap -x ava-ont --min-overlap 1000 --min-identity 0.99 --threads 4 {r1} {r1} >{paf}"]
    assert len(cmds) == 4 and not any("minimap2" in c or "fpa" in c for c in cmds)
    ov, paf, r1 = run(["--base", "--min-identity", "0.85", "--min-ovlplen-cns", "700", "--min-identity-cns", "0.98"])
    assert ov == [f"{py} -m vechat_amd.overlap -x ava-pb --min-identity 0.85 --threads 1 {rd} {rd} >{paf}",
                  f"{py} -m vechat_amd.overlap -x ava-pb --min-overlap 700 --min-identity 0.98 --threads 1 {r1} {r1} >{paf}"]
    ov, paf, _ = run(["--linear"])
    assert ov == [f"{py} -m vechat_amd.overlap -x ava-pb --threads 1 {rd} {rd} >{paf}"]      # one round, the round-1 command (scripts/vechat:36-38)
    # a template of the user's still wins, and the default is the reference's pipeline
    ov, _, _ = run(["--overlapper-r1", "MINE {targets} >{out}"])
    assert len(ov) == 1 and cmds[0].startswith("MINE ")
    del cmds[:]
    assert driver.main([str(reads), "-o", str(tmp_path / "out.fa"), "--workdir", str(tmp_path / "w2"), "--polisher", "POL"]) == 0
    assert cmds[0].startswith("minimap2 -x ava-pb") and cmds[2].startswith("minimap2 -cx ava-pb")
    with pytest.raises(SystemExit):
        driver.main([str(reads), "--overlapper", "mashmap"])
