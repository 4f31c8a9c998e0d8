"""The scrubber without a device: the CPU restatement of its rule (tests/scrub_ref.py) on the hand-built cases, the C ABI's argument
checks (which come before the device is touched), intervals_from_records, the naming of pieces and the report text, the command
line's arguments, the driver's --scrubber device command lines, and what the rule finds on simulated reads with spliced chimeras.
The device itself is pinned to the restatement in tests/test_scrub_gpu.py."""
import ctypes as C
import functools
import os
import shlex
import sys

import numpy as np
import pytest

import overlap_ref as OR
import scrub_cases as SC
import scrub_ref as R
from test_driver import simulate
from test_overlap import simulated
from vechat_amd import capi, driver, overlap, scrub

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def triples(res, kind):
    return [(int(r), int(b), int(e)) for r, b, e in zip(res[kind + "_read"], res[kind + "_begin"], res[kind + "_end"])]


def invariants(c, res):
    """what holds for every answer, whatever the case"""
    n = len(c["lengths"])
    reg, pcs = triples(res, "reg"), triples(res, "pc")
    assert reg == sorted(reg) and pcs == sorted(pcs)
    assert len(res["reg_off"]) == n + 1 and res["reg_off"][0] == 0 and res["reg_off"][-1] == len(reg)
    assert len(res["pc_off"]) == len(pcs) + 1 and [int(x) for x in np.diff(res["pc_off"].astype(np.int64))] == [e - b for _, b, e in pcs]
    for r in range(n):
        mine = reg[int(res["reg_off"][r]):int(res["reg_off"][r + 1])]
        assert all(x[0] == r and 0 <= x[1] < x[2] <= c["lengths"][r] for x in mine)
        assert all(a[2] < b[1] for a, b in zip(mine, mine[1:]))                # maximal runs: never adjacent
        assert int(res["bad_total"][r]) == sum(e - b for _, b, e in mine)
        if res["klass"][r] == R.NOT_COVERED:
            assert not any(p[0] == r for p in pcs)
        if res["klass"][r] == R.CLEAN:
            assert not mine


# ---------------------------------------------------------------------------------------------------- restatement
@functools.lru_cache(maxsize=None)
def restated(name, with_reads=True):
    c = SC.CASES[name]
    reads, quals = SC.reads_of(c["lengths"]) if with_reads else (None, None)
    return R.scrub(c["lengths"], c["intervals"], reads, quals, **c["params"])


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_restatement_on_the_case_table(name):
    c, res = SC.CASES[name], restated(name)
    invariants(c, res)
    if c["expect"] is not None:
        x = c["expect"]
        assert triples(res, "reg") == x["regions"]
        assert [int(k) for k in res["klass"]] == x["klass"]
        assert [int(t) for t in res["bad_total"]] == x["bad_total"]
        assert triples(res, "pc") == x["pieces"]
    reads, quals = SC.reads_of(c["lengths"])
    assert res["pc_bases"] == b"".join(reads[r][b:e] for r, b, e in triples(res, "pc"))
    assert res["pc_quals"] == b"".join(quals[r][b:e] for r, b, e in triples(res, "pc"))


def test_interval_order_does_not_matter_to_the_restatement():
    for name in ("region_left_right_inside_and_all_three", "adjacent_bad_segments_of_different_coverage", "nested_and_duplicate_intervals"):
        c = SC.CASES[name]
        want = restated(name)
        back = R.scrub(c["lengths"], c["intervals"][::-1], **c["params"])
        for f in ("reg_read", "reg_begin", "reg_end", "klass", "bad_total", "pc_read", "pc_begin", "pc_end"):
            assert np.array_equal(back[f], want[f]), (name, f)


def test_the_cut_case_takes_every_residue_and_length():
    """what the device test of k_scr_cut's heads and tails stands on: source and destination offsets of the pieces in every residue
    modulo 16, every length 1 .. 40, and pieces long enough for whole 16-byte chunks at every source residue"""
    c, res = SC.CASES["cut_every_residue_and_length"], restated("cut_every_residue_and_length")
    off = np.concatenate([[0], np.cumsum(c["lengths"])])
    pcs = triples(res, "pc")
    assert len(pcs) == 336
    assert {(int(off[r]) + b) % 16 for r, b, _ in pcs} == set(range(16))
    assert {int(x) % 16 for x in res["pc_off"][:-1]} == set(range(16))
    assert {e - b for _, b, e in pcs} >= set(range(1, 41))
    assert {(int(off[r]) + b) % 16 for r, b, e in pcs if e - b >= 100} == set(range(16))
    assert {(int(off[r]) + b) % 4 for r, b, e in pcs if e - b >= 100 and (int(off[r]) + b) % 16} == set(range(4))


def test_the_load_shape_case_is_lopsided():
    c, res = SC.CASES["one_read_with_thousands_of_intervals"], restated("one_read_with_thousands_of_intervals")
    per_read = np.bincount([r for r, _, _ in c["intervals"]], minlength=len(c["lengths"]))
    assert per_read.max() == 3000 and sorted(per_read)[-2] == 1 and len(c["lengths"]) == 301
    assert int(res["reg_off"][151]) - int(res["reg_off"][150]) >= 1                     # the deep read has regions of its own


def test_sweep_configurations_cover_the_parameters():
    cs = SC.sweep()
    assert len(cs) == 36
    for f, vals in (("coverage", {0, 1, 2, 3}), ("max_bad_permille", {0, 100, 400, 777, 1000}), ("min_piece", {1, 2, 10, 50})):
        assert {c["params"][f] for c in cs} == vals
    res = restated_sweep()
    for c, r in zip(cs, res):
        invariants(c, r)
    assert {int(k) for r in res for k in r["klass"]} == {0, 1, 2, 3}
    assert sum(1 for r in res if len(r["pc_read"])) >= 20 and sum(len(r["pc_read"]) for r in res) >= 50 and sum(len(r["reg_read"]) for r in res) >= 150
    assert any(0 in c["lengths"] for c in cs) and {c["with_reads"] for c in cs} == {c["with_quals"] for c in cs} == {False, True}


@functools.lru_cache(maxsize=None)
def restated_sweep():
    out = []
    for c in SC.sweep():
        reads, quals = SC.reads_of(c["lengths"], seed=2)
        out.append(R.scrub(c["lengths"], c["intervals"], reads if c["with_reads"] else None, quals if c["with_quals"] else None, **c["params"]))
    return tuple(out)


# ------------------------------------------------------------------------------------------- recall on simulated reads
ERR, SEED, N_SPLICED, COVERAGE = 0.06, 7, 6, 1


@functools.lru_cache(maxsize=None)
def spliced():
    """The 60 simulated reads of tests/test_overlap.py (3 kb from a 20 kb genome, nine-fold), N_SPLICED of them replaced by the first
    half of themselves joined to the second half of a read from a locus at least one read length away:
    (reads, {read: junction position})"""
    seqs, info, _ = simulated(ERR, seed=SEED)
    reads, junction, used = list(seqs), {}, set()
    for a in range(len(seqs)):
        if len(junction) == N_SPLICED:
            break
        if a in used or not 3500 <= info[a][0] <= 13500:                       # the chimera's own locus well inside the genome
            continue
        for b in range(len(seqs)):
            far = info[b][0] >= info[a][1] + 3000 or info[b][1] + 3000 <= info[a][0]
            if b != a and b not in used and b not in junction and far and 3500 <= info[b][0] <= 13500:
                ha, hb = len(seqs[a]) // 2, len(seqs[b]) // 2
                reads[a] = seqs[a][:ha] + seqs[b][hb:]
                junction[a] = ha
                used.update((a, b))
                break
    return tuple(reads), junction


@functools.lru_cache(maxsize=None)
def recall_figures():
    reads, junction = spliced()
    ov = OR.overlaps(list(reads), None, drop_internal=0)
    recs = [tuple(int(r[f]) for f in ("q_id", "q_begin", "q_end", "t_id", "t_begin", "t_end")) for r in ov]
    res = R.scrub([len(s) for s in reads], R.intervals_of(recs, dual=True), coverage=COVERAGE)
    reg = triples(res, "reg")
    found, worst = 0, 0
    for a, j in junction.items():
        hit = [(b, e) for r, b, e in reg if r == a and b <= j < e and b > 0 and e < len(reads[a])]
        if hit and res["klass"][a] == R.CHIMERIC:
            found += 1
            worst = max(worst, j - hit[0][0], hit[0][1] - j)
    split = sum(1 for r in range(len(reads)) if r not in junction and any(x[0] == r and x[1] > 0 and x[2] < len(reads[r]) for x in reg))
    slack = max(3 * int(r["block"]) // int(r["n_anchors"]) for r in ov if int(r["q_id"]) in junction)
    return dict(spliced=len(junction), found=found, worst=worst, split=split, slack=slack, records=len(ov),
                classes=[int(x) for x in np.bincount(res["klass"], minlength=4)])


RECORDED = dict(found=6, worst=81, split=0)          # profiles/scrub_recall.txt


def test_recall_on_simulated_reads_with_spliced_chimeras():
    """The rule itself, on the CPU, through the overlapper's restatement (drop_internal 0) and the scrubber's: every junction of a
    spliced read lies strictly inside a bad region of a read classed CHIMERIC, no unspliced read gets an interior region, and the
    region's ends lie no further from the junction than recorded plus the overlapper's end slack 3 * block / n_anchors (a chain ends
    at its outermost shared minimizer).  profiles/scrub_recall.txt records the figures."""
    f = recall_figures()
    print(f"{f['spliced']} spliced reads of 60, {f['records']} records, c = {COVERAGE}: {f['found']} junctions inside a bad region of a CHIMERIC read, "
          f"region ends at most {f['worst']} bp from the junction (end slack up to {f['slack']}), {f['split']} unspliced reads with an interior region, "
          f"classes clean / bad ends / chimeric / not covered {f['classes']}")
    assert f["spliced"] == N_SPLICED
    assert f["found"] >= RECORDED["found"]
    assert f["split"] <= RECORDED["split"]
    assert f["worst"] <= RECORDED["worst"] + f["slack"]


# ------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib(built):
    return capi.load_hip()


def test_header_exports_exist(lib):
    for sym in ("vc_scrub", "vc_scrub_default_params", "vc_scrub_last_error", "vc_scrub_release"):
        assert hasattr(lib, sym), sym
    p = scrub.default_params(lib)
    assert [p.device] + [getattr(p, f) for f in scrub.PARAMS] == [0, 0, 400, 1]
    header = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    for word in ("vc_scrub_params", "vc_scrub_in", "vc_scrub_out", "VC_SCRUB_NOT_COVERED 3", "1000 * bad_total > max_bad_permille * len",
                 "NOT a restatement of it", "cov_r(p) <= coverage"):
        assert word in header, word
    assert (scrub.CLEAN, scrub.BAD_ENDS, scrub.CHIMERIC, scrub.NOT_COVERED) == (R.CLEAN, R.BAD_ENDS, R.CHIMERIC, R.NOT_COVERED) == (0, 1, 2, 3)


NO_DEVICE = 9999       # an ordinal no machine has: what passes the argument checks ends as VC_ERR_NO_DEVICE, with or without a GPU


def test_arguments_are_checked_before_the_device_in_the_documented_order(lib):
    scrub.declare(lib)
    u32 = lambda v: np.array(v, np.uint32)
    u64 = lambda v: np.array(v, np.uint64)
    arrays = dict(len=u32([100, 50]), read=u32([0, 1]), begin=u32([0, 10]), end=u32([100, 50]), off=u64([0, 100, 150]),
                  bases=np.frombuffer(b"A" * 151, np.uint8).copy(), quals=np.frombuffer(b"5" * 151, np.uint8).copy())
    kinds = dict(len=C.c_uint32, read=C.c_uint32, begin=C.c_uint32, end=C.c_uint32, off=C.c_uint64, bases=C.c_uint8, quals=C.c_uint8)
    out = scrub.VcScrubOut()

    def call(n=2, m=2, params=None, **replace):
        """one call with the good arrays, some replaced (None: a NULL pointer)"""
        use = dict(arrays, **replace)
        ptr = {k: (use[k].ctypes.data_as(C.POINTER(kinds[k])) if use[k] is not None else None) for k in kinds}
        a = scrub.VcScrubIn(n, ptr["len"], m, ptr["read"], ptr["begin"], ptr["end"], ptr["off"], ptr["bases"], ptr["quals"])
        p = scrub.default_params(lib, device=NO_DEVICE, **(params or {}))
        rc = lib.vc_scrub(C.byref(p), C.byref(a), C.byref(out))
        assert not out.reg_read and not out.reg_off and not out.pc_off and out.n_regions == 0          # a failed call leaves every pointer NULL
        return rc, lib.vc_scrub_last_error().decode()

    assert call()[0] == capi.VC_ERR_NO_DEVICE                    # everything in order: only the device is missing
    assert call(off=None, bases=None, quals=None)[0] == capi.VC_ERR_NO_DEVICE
    assert call(quals=None)[0] == capi.VC_ERR_NO_DEVICE          # a read set without qualities is legal
    assert call(n=0, m=0)[0] == capi.VC_ERR_NO_DEVICE
    p = scrub.default_params(lib, device=NO_DEVICE)
    a = scrub.VcScrubIn()
    assert lib.vc_scrub(None, C.byref(a), C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_scrub(C.byref(p), None, C.byref(out)) == capi.VC_ERR_ARG
    assert lib.vc_scrub(C.byref(p), C.byref(a), None) == capi.VC_ERR_ARG
    # one condition at a time, each VC_ERR_ARG.  The read beyond the envelope is checked on its length alone: its bases are never read
    long_read = dict(len=u32([100, (1 << 30) + 1]), off=u64([0, 100, 101 + (1 << 30)]))
    for kw in (dict(len=None), dict(read=None), dict(begin=None), dict(end=None), dict(off=None), dict(bases=None), dict(off=u64([1, 100, 150])),
               dict(off=u64([0, 160, 150])), dict(off=u64([0, 90, 150])), dict(params=dict(coverage=-1)), dict(params=dict(coverage=(1 << 30) + 1)),
               dict(params=dict(max_bad_permille=-1)), dict(params=dict(max_bad_permille=1001)), dict(params=dict(min_piece=0)),
               dict(read=u32([0, 2])), dict(begin=u32([0, 50])), dict(begin=u32([0, 51])), dict(end=u32([101, 50])), dict(end=u32([100, 51])), long_read):
        rc, msg = call(**kw)
        assert rc == capi.VC_ERR_ARG and msg, kw
    # the order: NULL pointers, offsets, parameters, intervals, the envelope -- the earlier one is the one reported
    order = [(dict(read=None), "NULL"), (dict(off=u64([1, 100, 150])), "start at 0"), (dict(params=dict(min_piece=0)), "min_piece"),
             (dict(end=u32([101, 50])), "outside its read"), (long_read, "envelope")]
    for i, (kw, word) in enumerate(order):
        assert word in call(**kw)[1], (kw, word)
        for later, _ in order[i + 1:]:
            assert word in call(**dict(later, **kw))[1], (kw, later)
    # within the parameters and within an interval: the order of the header
    assert "coverage" in call(params=dict(coverage=-1, max_bad_permille=2000, min_piece=0))[1]
    assert "not there" in call(read=u32([0, 7]), begin=u32([0, 60]))[1]
    assert "empty" in call(begin=u32([0, 50]), end=u32([100, 50]))[1]
    lib.vc_scrub_release()


# -------------------------------------------------------------------------------- intervals, names, report, arguments
def test_intervals_from_records_in_both_modes():
    recs = np.zeros(3, overlap.RECORD)
    recs[0] = (1, 0, 0, 5, 905, 100, 1000, 60, 850, 880, 900)
    recs[1] = (0, 1, 1, 100, 1000, 5, 905, 60, 850, 880, 900)
    recs[2] = (2, 0, 1, 0, 700, 20, 725, 40, 600, 650, 705)
    rows = [tuple(int(r[f]) for f in ("q_id", "q_begin", "q_end", "t_id", "t_begin", "t_end")) for r in recs]
    dual = scrub.intervals_from_records(recs, dual=True)
    assert dual.shape == (3, 3) and [tuple(x) for x in dual.tolist()] == [(1, 5, 905), (0, 100, 1000), (2, 0, 700)] == R.intervals_of(rows, True)
    both = scrub.intervals_from_records(recs, dual=False)
    assert [tuple(x) for x in both.tolist()] == [(1, 5, 905), (0, 100, 1000), (0, 100, 1000), (1, 5, 905), (2, 0, 700), (0, 20, 725)] == R.intervals_of(rows, False)
    assert scrub.intervals_from_records(recs[:0], dual=True).shape == (0, 3) and scrub.intervals_from_records(recs[:0], dual=False).shape == (0, 3)
    cols = {f: [3, 4] for f in ("q_id", "t_id")}
    cols.update(q_begin=[0, 1], q_end=[9, 8], t_begin=[2, 3], t_end=[7, 6])
    assert scrub.intervals_from_records(cols, dual=False).tolist() == [[3, 0, 9], [3, 2, 7], [4, 1, 8], [4, 3, 6]]


def test_piece_names_and_report_text(tmp_path):
    """the naming rule and the report line, from the package's formatters and the restatement's, on an answer written out by hand"""
    names, headers = ["r0", "r1", "r2", "r3"], ["r0 whole read", "r1 cut=here", "r2", "r3 dropped"]
    reads, quals = [b"ACGTACGTAC", b"AAAACCCCGGGGTTTT", b"GATTACA", b"TTTT"], [b"0123456789", b"abcdefghijklmnop", b"ABCDEFG", b"!!!!"]
    res = dict(pc_read=np.array([0, 1, 1, 2], np.uint32), pc_begin=np.array([0, 0, 12, 1], np.uint32), pc_end=np.array([10, 4, 16, 7], np.uint32),
               reg_off=np.array([0, 0, 1, 2, 3], np.uint64), reg_begin=np.array([4, 0, 0], np.uint32), reg_end=np.array([12, 1, 4], np.uint32),
               klass=np.array([0, 2, 1, 3], np.uint8))
    pieces = [(None, b"ACGTACGTAC", b"0123456789"), ("_0_4", b"AAAA", b"abcd"), ("_12_16", b"TTTT", b"mnop"), ("_1_7", b"ATTACA", b"BCDEFG")]
    fq = "@r0 whole read\nACGTACGTAC\n+\n0123456789\n@r1_0_4\nAAAA\n+\nabcd\n@r1_12_16\nTTTT\n+\nmnop\n@r2_1_7\nATTACA\n+\nBCDEFG\n"
    assert scrub.format_pieces(pieces, res, names, headers, True) == fq == R.format_reads(names, headers, reads, quals, res)
    fa = ">r0 whole read\nACGTACGTAC\n>r1_0_4\nAAAA\n>r1_12_16\nTTTT\n>r2_1_7\nATTACA\n"
    assert scrub.format_pieces([(s, b, None) for s, b, _ in pieces], res, names, headers, False) == fa == R.format_reads(names, headers, reads, None, res)
    report = "Chimeric\tr1\t16\t8,4,12\nBadEnds\tr2\t7\t1,0,1\nNotCovered\tr3\t4\t4,0,4\n"
    assert scrub.format_report(names, [10, 16, 7, 4], res) == report == R.format_report(names, [10, 16, 7, 4], res)
    path = tmp_path / "h.fq"
    path.write_text("@r0 whole read\nACGT\n+\n@@@@\n@r1 cut=here\nAC\n+\n>>\n")
    assert scrub.read_headers(str(path)) == ["r0 whole read", "r1 cut=here"]
    path = tmp_path / "h.fa"
    path.write_text(">r0 whole read\nACGT\nACGT\n>r1\nAC\n")
    assert scrub.read_headers(str(path)) == ["r0 whole read", "r1"]


def test_command_line_arguments(capsys):
    a = scrub.parse_args(["reads.fq"])
    assert (a.preset, a.coverage, a.max_bad_permille, a.max_gap, a.min_piece, a.paf, a.report, a.out, a.reads) == ("ava-ont", 0, 400, 5000, 1, None, None, "-", "reads.fq")
    a = scrub.parse_args(["-x", "ava-pb", "-c", "3", "-n", "0.4", "-g", "500", "--min-piece", "200", "--paf", "o.paf", "--report", "r.txt", "-o", "out.fq", "reads.fq"])
    assert (a.preset, a.coverage, a.max_bad_permille, a.max_gap, a.min_piece, a.paf, a.report, a.out) == ("ava-pb", 3, 400, 500, 200, "o.paf", "r.txt", "out.fq")
    assert [scrub.parse_args(["-n", f, "r"]).max_bad_permille for f in ("0", "0.0005", "0.0015", "0.3333", "0.29", "1")] == [0, 0, 2, 333, 290, 1000]
    for bad in (["-x", "map-ont", "r"], ["-c", "-1", "r"], ["-n", "1.5", "r"], ["-g", "0", "r"], ["--min-piece", "0", "r"], []):
        with pytest.raises(SystemExit):
            scrub.parse_args(bad)
    with pytest.raises(SystemExit):
        scrub.parse_args(["--help"])
    assert "not a restatement" in " ".join(capsys.readouterr().out.split())
    with pytest.raises(TypeError):
        scrub.default_params(None, no_such_field=1)


# -------------------------------------------------------------------------------------------------------- driver
def test_driver_scrubber_device_command_lines(tmp_path, monkeypatch):
    cmds = []

    def fake_sh(cmd, cwd):                                     # no tool runs: a scrub command's reads are the input's, the other outputs appear empty
        cmds.append(cmd)
        a = shlex.split(cmd)
        if "vechat_amd.scrub" in cmd:                          # ... -o OUT reads
            open(a[-2], "w").write(open(a[-1]).read())
        elif cmd.startswith("yacrd"):                          # ... scrubb -i reads -o OUT
            open(a[-1], "w").write(open(a[-3]).read())
        else:
            open(os.path.join(cwd, cmd.rsplit(">", 1)[1].strip().strip("'")), "w").close()

    monkeypatch.setattr(driver, "_sh", fake_sh)
    py = shlex.quote(sys.executable)

    def run(extra, fastq=True):
        del cmds[:]
        reads = tmp_path / ("reads.fastq" if fastq else "reads.fasta")
        simulate(str(reads), n_reads=4, fastq=fastq)
        work = tmp_path / "work"
        assert driver.main([str(reads), "-o", str(tmp_path / "out.fa"), "--workdir", str(work), "--polisher", "POL", "--scrub"] + extra) == 0
        return shlex.quote(str(reads)), work

    rd, work = run(["--overlapper", "device", "--scrubber", "device", "--platform", "ont", "-t", "4"])
    sc = shlex.quote(str(work / "reads.scrubbed.fq"))
    assert cmds[0] == f"{py} -m vechat_amd.scrub -x ava-ont -g 500 -c 4 -n 0.4 --report {shlex.quote(str(work / 'report.yacrd'))} -o {sc} {rd}"
    assert cmds[1] == f"{py} -m vechat_amd.overlap -x ava-ont --threads 4 {sc} {sc} >{shlex.quote(str(work / 'overlap.paf'))}"
    assert len(cmds) == 5 and not any("minimap2" in c or c.startswith("yacrd") or "fpa" in c for c in cmds)
    rd, work = run(["--overlapper", "device", "--scrubber", "device", "--linear"], fastq=False)
    sc = shlex.quote(str(work / "reads.scrubbed.fa"))
    assert cmds[0] == f"{py} -m vechat_amd.scrub -x ava-pb -g 5000 -c 3 -n 0.4 --report {shlex.quote(str(work / 'report.yacrd'))} -o {sc} {rd}"
    assert len(cmds) == 3
    # the scrubber alone: the overlaps of the rounds stay minimap2's
    rd, work = run(["--scrubber", "device"])
    assert "vechat_amd.scrub" in cmds[0] and cmds[1].startswith("minimap2 -x ava-pb --dual=yes")
    # the default, and --overlapper device without --scrubber device: the reference's two commands, as they were
    for extra in ([], ["--overlapper", "device"], ["--scrubber", "yacrd"]):
        rd, work = run(extra)
        assert cmds[0] == f"minimap2 -x ava-pb -g 5000 -t 1 {rd} {rd} > {shlex.quote(str(work / 'scrub.paf'))}"
        assert cmds[1] == (f"yacrd -i {shlex.quote(str(work / 'scrub.paf'))} -o {shlex.quote(str(work / 'report.yacrd'))} -c 3 -n 0.4 scrubb -i {rd} "
                           f"-o {shlex.quote(str(work / 'reads.scrubbed.fq'))}")
    with pytest.raises(SystemExit):
        driver.main(["reads.fq", "--scrubber", "porechop"])
