"""The demultiplexer without a device: the CPU restatement of its rule (tests/demux_ref.py) on the hand-built cases, its independence
of read order and pattern order, the C ABI's argument checks (which come before the device is touched), read_patterns, the report
text, the command line's arguments, and what the rule finds on simulated barcoded reads with errors.  The device itself is pinned
to the restatement in tests/test_demux_gpu.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import demux_cases as DC
import demux_ref as R
from vechat_amd import capi, demux

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = ("v_pat", "v_dist", "v_start", "v_end", "v_second", "klass", "label", "flip", "begin", "end", "piece_off", "grp_off", "grp_reads")


def run_ref(c):
    return R.demux(c["reads"], c["patterns"], c["labels"], c["sides"], c["quals"], **c["params"])


@functools.lru_cache(maxsize=None)
def restated(name):
    return run_ref(DC.CASES[name])


@functools.lru_cache(maxsize=None)
def restated_sweep():
    return tuple(run_ref(c) for c in DC.sweep())


def check_expect(c, res):
    """the answers written out by hand: whole lists, or {index: value}"""
    for f, want in c["expect"].items():
        if isinstance(want, dict):
            for i, x in want.items():
                assert int(res[f][i]) == x, (f, i, int(res[f][i]), x)
        elif isinstance(want, bytes):
            assert res[f] == want, (f, res[f], want)
        else:
            assert [int(x) for x in res[f]] == want, (f, [int(x) for x in res[f]], want)


def invariants(c, res):
    """what holds for every answer, whatever the case"""
    n, P = len(c["reads"]), len(c["patterns"])
    labels = c["labels"] if c["labels"] is not None else list(range(P))
    assert all(len(res[f]) == 2 * n for f in FIELDS[:5]) and all(len(res[f]) == n for f in FIELDS[5:10]) and len(res["piece_off"]) == n + 1
    for r, read in enumerate(c["reads"]):
        assert 0 <= res["begin"][r] <= res["end"][r] <= len(read)
        assert int(res["piece_off"][r + 1]) - int(res["piece_off"][r]) == int(res["end"][r]) - int(res["begin"][r])
        assert (res["label"][r] != R.UNASSIGNED) == (res["klass"][r] == R.BOTH_ENDS or (res["klass"][r] == R.ONE_END and not c["params"].get("flags", 0) & R.REQUIRE_BOTH))
        for v in (2 * r, 2 * r + 1):
            if res["v_pat"][v] == R.UNASSIGNED:
                assert (res["v_dist"][v], res["v_start"][v], res["v_end"][v], res["v_second"][v]) == (255, 0, 0, 255)
            else:
                m = len(c["patterns"][int(res["v_pat"][v])])
                assert 1000 * int(res["v_dist"][v]) <= c["params"].get("max_err_permille", 200) * m
                assert res["v_start"][v] <= res["v_end"][v] <= min(len(read), c["params"].get("window", 150)) and res["v_second"][v] >= res["v_dist"][v]
                assert abs(int(res["v_end"][v]) - int(res["v_start"][v]) - m) <= res["v_dist"][v]
    assert len(res["grp_off"]) == (1 + max(labels) if P else 0) + 1 and res["grp_off"][0] == 0 and res["grp_off"][-1] == len(res["grp_reads"])
    want = sorted((int(res["label"][r]), r) for r in range(n) if res["label"][r] != R.UNASSIGNED)
    assert [int(r) for r in res["grp_reads"]] == [r for _, r in want]
    assert len(res["pc_bases"]) == res["piece_off"][-1] and (res["pc_quals"] is None) == (c["quals"] is None)
    if c["params"].get("flags", 0) & R.ALL_HITS:
        assert len(res["all_dist"]) == len(res["all_end"]) == 2 * n * P
    else:
        assert res["all_dist"] is None and res["all_end"] is None


# ---------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_restatement_on_the_case_table(name):
    c, res = DC.CASES[name], restated(name)
    invariants(c, res)
    check_expect(c, res)


def test_the_case_table_covers_what_it_should():
    cs = DC.CASES
    assert {len(p) for c in cs.values() for p in c["patterns"]} >= {1, 31, 32, 33, 63, 64}
    assert {len(c["patterns"]) for c in cs.values()} >= {1, 63, 64, 65}
    assert {c["params"].get("trim", 1) for c in cs.values()} == {0, 1, 2} and {c["params"].get("min_margin", 2) for c in cs.values()} >= {0, 1, 2}
    assert {c["params"].get("max_err_permille", 200) for c in cs.values()} >= {0, 200, 1000} and any(c["params"].get("window") == 1 for c in cs.values())
    assert {int(k) for name in cs for k in restated(name)["klass"]} == {0, 1, 2, 3, 4}
    assert any(0 in [len(r) for r in c["reads"]] for c in cs.values()) and any(c["quals"] for c in cs.values())
    assert 18 * 65 > 4 * 256                                                     # patterns_65: its triples fill more than four blocks


def test_read_order_and_pattern_order_do_not_matter():
    """reads are independent; patterns in another order give the same answer up to the tie rule's `smaller j`, which no pattern of
    these cases needs (no two accepted hits of a view with equal distance and equal length)"""
    for name in ("every_class", "plus_and_minus_evidence", "one_error_apart_is_ambiguous_at_margin_2_only"):
        c, want = DC.CASES[name], restated(name)
        n, P = len(c["reads"]), len(c["patterns"])
        labels, sides = c["labels"] or list(range(P)), c["sides"] or [0] * P
        back = R.demux(c["reads"][::-1], c["patterns"], labels, sides, **c["params"])
        for f in ("klass", "label", "flip", "begin", "end"):
            assert np.array_equal(back[f][::-1], want[f]), (name, f)
        for f in FIELDS[:5]:
            assert np.array_equal(back[f].reshape(n, 2)[::-1].reshape(-1), want[f]), (name, f)
        perm = [(j + 1) % P for j in range(P)]
        turned = R.demux(c["reads"], [c["patterns"][j] for j in perm], [labels[j] for j in perm], [sides[j] for j in perm], **c["params"])
        for f in ("klass", "label", "flip", "begin", "end", "v_dist", "v_start", "v_end", "v_second", "grp_off", "grp_reads"):
            assert np.array_equal(turned[f], want[f]), (name, f)
        assert [perm[int(p)] if p != R.UNASSIGNED else p for p in turned["v_pat"]] == [int(p) for p in want["v_pat"]]


def test_sweep_configurations_cover_the_parameters():
    cs = DC.sweep()
    assert len(cs) == 20 and sum(len(c["reads"]) for c in cs) == 200
    assert {(len(c["patterns"]), c["params"]["window"]) for c in cs} == {(P, w) for P in (1, 7, 64, 65, 130) for w in (1, 33, 150, 600)}
    assert {c["params"]["trim"] for c in cs} == {0, 1, 2} and {c["params"]["flags"] & 3 for c in cs} == {0, 1, 2, 3} and any(c["params"]["flags"] & 4 for c in cs)
    res = restated_sweep()
    for c, r in zip(cs, res):
        invariants(c, r)
    assert {int(k) for r in res for k in r["klass"]} == {0, 1, 2, 3, 4}
    assert max(len(x) for c in cs for x in c["reads"]) > 550 and min(len(x) for c in cs for x in c["reads"]) == 0


# ------------------------------------------------------------------------------------------ recall on simulated reads
N_BARCODES, N_READS, ERR, SEED = 24, 400, 0.08, 3


@functools.lru_cache(maxsize=None)
def barcoded():
    """24 seeded barcodes of 24 bases; 400 reads of 400..800 bases, each with its barcode in front and the barcode's reverse
    complement behind, on a random strand, and then ERR errors per base over the whole read (a third each substitutions, insertions
    and deletions): (barcodes, reads, the barcode of every read)"""
    rng = np.random.default_rng(SEED)
    barcodes = [DC.random_bases(rng, 24) for _ in range(N_BARCODES)]
    reads, truth = [], []
    for _ in range(N_READS):
        b = int(rng.integers(N_BARCODES))
        clean = barcodes[b] + DC.random_bases(rng, int(rng.integers(400, 801)) - 48) + DC.rc(barcodes[b])
        if rng.random() < 0.5:
            clean = DC.rc(clean)
        noisy = bytearray()
        for ch in clean:
            x = rng.random()
            if x < ERR / 3:
                noisy.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            elif x < 2 * ERR / 3:
                noisy.append(ch); noisy.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            elif x >= ERR:
                noisy.append(ch)
        reads.append(bytes(noisy)); truth.append(b)
    return barcodes, reads, truth


@functools.lru_cache(maxsize=None)
def recall_result():
    barcodes, reads, _ = barcoded()
    return R.demux(reads, barcodes)


def recall_figures():
    _, reads, truth = barcoded()
    res = recall_result()
    label, klass = res["label"], res["klass"]
    correct = sum(1 for r in range(len(reads)) if label[r] == truth[r])
    wrong = sum(1 for r in range(len(reads)) if label[r] != R.UNASSIGNED and label[r] != truth[r])
    ambiguous = sum(1 for r in range(len(reads)) if klass[r] in (R.AMBIGUOUS, R.CONFLICT))
    missed = sum(1 for r in range(len(reads)) if klass[r] == R.NONE)
    return dict(correct=correct, wrong=wrong, ambiguous=ambiguous, missed=missed, both=int((klass == R.BOTH_ENDS).sum()), one=int((klass == R.ONE_END).sum()))


RECORDED = dict(correct=400, wrong=0)                        # profiles/demux_recall.txt


def test_recall_on_simulated_barcoded_reads():
    """The rule itself, on the CPU, through the restatement at the default parameters: how many of 400 reads with 8 % errors per
    base get their own barcode, another one, an ambiguous or contradictory answer, or none.  profiles/demux_recall.txt records the
    figures; correct is held from below and wrong from above."""
    f = recall_figures()
    print(f"{N_READS} reads of 400..800 bases, {N_BARCODES} barcodes of 24 bases on both ends, {ERR:.0%} errors per base, random strand, defaults: "
          f"{f['correct']} correct ({f['both']} at both ends, {f['one']} at one), {f['wrong']} wrong, {f['ambiguous']} ambiguous or conflicting, {f['missed']} missed")
    assert f["correct"] + f["wrong"] + f["ambiguous"] + f["missed"] == N_READS
    assert f["correct"] >= RECORDED["correct"]
    assert f["wrong"] <= RECORDED["wrong"]


# ------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib(built):
    return capi.load_hip()


def test_header_exports_exist(lib):
    for sym in ("vc_demux", "vc_demux_default_params", "vc_demux_last_error", "vc_demux_release"):
        assert hasattr(lib, sym), sym
    p = demux.default_params(lib)
    assert [p.device] + [getattr(p, f) for f in demux.PARAMS] == [0, 150, 200, 2, 1, 0]
    assert demux.PARAMS == ("window", "max_err_permille", "min_margin", "trim", "flags") and C.sizeof(capi.VcDemuxParams) == 24
    header = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    for word in ("vc_demux_params", "vc_demux_in", "vc_demux_out", "VC_DEMUX_AMBIGUOUS  4", "VC_DEMUX_MAX_LABELS   0x100000u", "1000 * d <= max_err_permille * m",
                 "a restatement of neither", "flip = minus && !plus", "VC_DEMUX_BUDGET_MB"):
        assert word in header, word
    assert (demux.NONE, demux.ONE_END, demux.BOTH_ENDS, demux.CONFLICT, demux.AMBIGUOUS) == (R.NONE, R.ONE_END, R.BOTH_ENDS, R.CONFLICT, R.AMBIGUOUS) == (0, 1, 2, 3, 4)
    assert (demux.REQUIRE_BOTH, demux.ORIENT, demux.ALL_HITS, demux.UNASSIGNED) == (R.REQUIRE_BOTH, R.ORIENT, R.ALL_HITS, R.UNASSIGNED) == (1, 2, 4, 0xFFFFFFFF)
    assert (demux.ANY, demux.HEAD, demux.TAIL) == (R.ANY, R.HEAD, R.TAIL) == (0, 1, 2)


NO_DEVICE = 9999       # an ordinal no machine has: what passes the argument checks ends as VC_ERR_NO_DEVICE, with or without a GPU


def test_arguments_are_checked_before_the_device_in_the_documented_order(lib):
    demux.declare(lib)
    u8 = lambda v: np.frombuffer(bytes(v), np.uint8).copy()
    u32 = lambda v: np.array(v, np.uint32)
    u64 = lambda v: np.array(v, np.uint64)
    arrays = dict(off=u64([0, 100, 150]), bases=u8(b"A" * 151), quals=u8(b"5" * 151), pat_off=u64([0, 4, 10]), pat_bases=u8(b"ACGTACGTNN\0"), label=u32([0, 3]),
                  side=u8([0, 2]))
    kinds = dict(off=C.c_uint64, bases=C.c_uint8, quals=C.c_uint8, pat_off=C.c_uint64, pat_bases=C.c_uint8, label=C.c_uint32, side=C.c_uint8)
    out = demux.VcDemuxOut()

    def call(n=2, P=2, params=None, **replace):
        """one call with the good arrays, some replaced (None: a NULL pointer)"""
        use = dict(arrays, **replace)
        ptr = {k: (use[k].ctypes.data_as(C.POINTER(kinds[k])) if use[k] is not None else None) for k in kinds}
        a = demux.VcDemuxIn(n, ptr["off"], ptr["bases"], ptr["quals"], P, ptr["pat_off"], ptr["pat_bases"], ptr["label"], ptr["side"])
        p = demux.default_params(lib, device=NO_DEVICE, **(params or {}))
        rc = lib.vc_demux(C.byref(p), C.byref(a), C.byref(out))
        assert not out.v_pat and not out.piece_off and not out.grp_off and not out.pc_bases and out.n_reads == 0      # a failed call leaves every pointer NULL
        return rc, lib.vc_demux_last_error().decode()

    assert call()[0] == capi.VC_ERR_NO_DEVICE                    # everything in order: only the device is missing
    assert call(quals=None)[0] == capi.VC_ERR_NO_DEVICE          # a read set without qualities is legal
    assert call(n=0, off=None, bases=None, quals=None)[0] == capi.VC_ERR_NO_DEVICE
    assert call(n=0, P=0, off=None, bases=None, quals=None, pat_off=None, pat_bases=None, label=None, side=None)[0] == capi.VC_ERR_NO_DEVICE
    p = demux.default_params(lib, device=NO_DEVICE)
    a = demux.VcDemuxIn()
    assert lib.vc_demux(None, C.byref(a), C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_demux(C.byref(p), None, C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_demux(C.byref(p), C.byref(a), None) == capi.VC_ERR_ARG
    # one condition at a time, each VC_ERR_ARG.  The read beyond the envelope is checked on its length alone: its bases are never read
    long_read = dict(off=u64([0, 100, 101 + (1 << 30)]))
    for kw in (dict(off=None), dict(bases=None), dict(pat_off=None), dict(pat_bases=None), dict(label=None), dict(side=None), dict(off=u64([1, 100, 150])),
               dict(off=u64([0, 160, 150])), dict(pat_off=u64([1, 4, 10])), dict(pat_off=u64([0, 11, 10])), dict(params=dict(window=0)), dict(params=dict(window=4097)),
               dict(params=dict(max_err_permille=-1)), dict(params=dict(max_err_permille=1001)), dict(params=dict(min_margin=-1)), dict(params=dict(min_margin=65)),
               dict(params=dict(trim=3)), dict(params=dict(trim=-1)), dict(params=dict(flags=8)), dict(P=0), dict(pat_off=u64([0, 0, 10])),
               dict(pat_off=u64([0, 4, 69]), pat_bases=u8(b"A" * 70)), dict(pat_bases=u8(b"ACGTACGTNn\0")), dict(pat_bases=u8(b"ACGUACGTNN\0")), dict(side=u8([0, 3])),
               dict(label=u32([0, 1 << 20])), long_read):
        rc, msg = call(**kw)
        assert rc == capi.VC_ERR_ARG and msg, kw
    assert call(pat_off=u64([0, 4, 68]), pat_bases=u8(b"A" * 69))[0] == capi.VC_ERR_NO_DEVICE        # a pattern of 64 is legal
    assert call(label=u32([0, (1 << 20) - 1]))[0] == capi.VC_ERR_NO_DEVICE
    # the order: NULL pointers, read offsets, pattern offsets, parameters, no pattern, the patterns, the envelope
    order = [(dict(side=None), "NULL"), (dict(off=u64([1, 100, 150])), "read offsets do not start"), (dict(pat_off=u64([0, 11, 10])), "pattern offsets decrease"),
             (dict(params=dict(trim=3)), "trim"), (dict(side=u8([0, 3])), "side above 2"), (long_read, "envelope")]
    for i, (kw, word) in enumerate(order):
        assert word in call(**kw)[1], (kw, word)
        for later, _ in order[i + 1:]:
            assert word in call(**dict(later, **kw))[1], (kw, later)
    assert "without a pattern" in call(P=0, params=dict())[1] and "trim" in call(P=0, params=dict(trim=3))[1]
    # within the parameters and within a pattern: the order of the header
    assert "window" in call(params=dict(window=0, max_err_permille=2000, min_margin=-1, trim=5, flags=64))[1]
    assert "length" in call(pat_off=u64([0, 0, 10]), side=u8([3, 3]), label=u32([1 << 20, 0]))[1]
    assert "IUPAC" in call(pat_bases=u8(b"ACGTACGTNn\0"), side=u8([0, 3]))[1] and "side" in call(side=u8([0, 3]), label=u32([0, 1 << 20]))[1]
    lib.vc_demux_release()


# ------------------------------------------------------------------------------------- patterns, report, arguments
def test_read_patterns(tmp_path):
    path = tmp_path / "p.fa"
    path.write_text(">bc01:head\nACGT\n>bc02\nGGNN\nRY\n>bc01:tail\nttaa\n>amp:x:any\nA\n")
    patterns, labels, sides, label_names, pattern_names = demux.read_patterns(str(path))
    assert patterns == [b"ACGT", b"GGNNRY", b"TTAA", b"A"] and labels == [0, 1, 0, 2] and sides == [demux.HEAD, demux.ANY, demux.TAIL, demux.ANY]
    assert label_names == ["bc01", "bc02", "amp:x"] and pattern_names == ["bc01:head", "bc02", "bc01:tail", "amp:x:any"]
    (tmp_path / "bad.fa").write_text(">bc01:left\nACGT\n")
    with pytest.raises(ValueError, match="label_name"):
        demux.read_patterns(str(tmp_path / "bad.fa"))


def test_report_text_and_groups():
    """the report line and the groups, from the package's formatters and the restatement's, on an answer written out by hand"""
    c = DC.CASES["plus_and_minus_evidence"]
    res = restated("plus_and_minus_evidence")
    names = [f"r{i}" for i in range(len(c["reads"]))]
    text = demux.format_report(names, ["amp"], ["amp:head", "amp:tail"], res)
    assert text == R.format_report(names, ["amp"], ["amp:head", "amp:tail"], res)
    lines = text.split("\n")
    assert lines[0] == "r0\tBothEnds\tamp\t+\t24\t90\tamp:head\t0\t0\t24\tamp:tail\t0\t0\t24"
    assert lines[1] == "r1\tBothEnds\tamp\t-\t24\t90\tamp:tail\t0\t0\t24\tamp:head\t0\t0\t24"
    assert lines[5] == "r5\tOneEnd\tamp\t-\t0\t60\t*\t*\t*\t*\tamp:head\t0\t0\t24" and lines[6].startswith("r6\tConflict\t*\t+\t24\t84\t")
    got = demux.DemuxResult(res, flags=0)
    groups = demux.groups_of(got, c["reads"])                 # not oriented on the device: flipped here
    assert groups == [[c["reads"][0][24:90], DC.rc(c["reads"][1][24:90]), c["reads"][2][24:], DC.rc(c["reads"][3][24:]), c["reads"][4][:60], DC.rc(c["reads"][5][:60])]]
    assert groups[0][0] == groups[0][1]
    oriented = R.demux(c["reads"], c["patterns"], c["labels"], c["sides"], flags=R.ORIENT)
    assert demux.groups_of(demux.DemuxResult(oriented, flags=R.ORIENT), c["reads"]) == groups == R.groups_of(oriented)
    assert demux.format_reads(names, ["amp"], got, [0, 6], True) == f">r0 label=amp\n{c['reads'][0][24:90].decode()}\n>r6\n{c['reads'][6][24:84].decode()}\n"
    assert demux.format_consensus(["a", "b", "c"], [[b"A"], [], [b"C", b"C"]], [b"AC", b"GT"]) == ">a size=1\nAC\n>c size=2\nGT\n"


def test_command_line_arguments(capsys):
    a = demux.parse_args(["p.fa", "reads.fq"])
    assert a.params == dict(window=150, max_err_permille=200, min_margin=2, trim=1, require_both=False, orient=False)
    assert (a.report, a.out_dir, a.out, a.unassigned, a.consensus, a.algorithm, a.patterns, a.reads) == (None, None, None, None, None, 1, "p.fa", "reads.fq")
    a = demux.parse_args(["-w", "80", "-e", "0.15", "--min-margin", "3", "--trim", "2", "--both-ends", "--orient", "--report", "r.tsv", "--out-dir", "d", "--unassigned",
                          "u.fq", "--consensus", "c.fa", "-l", "2", "p.fa", "reads.fq"])
    assert a.params == dict(window=80, max_err_permille=150, min_margin=3, trim=2, require_both=True, orient=True)
    assert (a.report, a.out_dir, a.out, a.unassigned, a.consensus, a.algorithm) == ("r.tsv", "d", None, "u.fq", "c.fa", 2)
    for bad in (["-w", "0", "p", "r"], ["-w", "4097", "p", "r"], ["-e", "1.5", "p", "r"], ["--min-margin", "65", "p", "r"], ["--trim", "3", "p", "r"],
                ["--out-dir", "d", "-o", "f", "p", "r"], ["p"], []):
        with pytest.raises(SystemExit):
            demux.parse_args(bad)
    with pytest.raises(SystemExit):
        demux.parse_args(["--help"])
    assert "not a restatement" in " ".join(capsys.readouterr().out.split())
    with pytest.raises(TypeError):
        demux.default_params(None, no_such_field=1)
