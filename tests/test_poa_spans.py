"""CPU suite: span-limited alignment of POA group members (vc_poa_run_spans, the spans= keyword of vechat_amd.poa, racon_spans, the
command line's --spans) at its boundary -- declared, exported and bound, the arguments refused before the device, the parser --
and the CPU restatement tests/poa_spans_ref.py, the live bar for the device, against every entry of
tests/golden/poa_spans.json.gz (spoa's own Subgraph / UpdateAlignment / AddAlignment loop)."""
import ctypes as C
import gzip
import hashlib
import json
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import oracle_api as oa
import poa_graph_ref as G
import poa_msa_ref as pm
import poa_spans_ref as SR
import poa_strand_ref as S
from poa_common import _gp, _workers
from test_poa import _device_visible, load_fixture
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = capi.VC_POA_SPAN_NONE
_FX = {}


def load_spans_fixture():
    if not _FX:
        _FX.update(json.load(gzip.open(os.path.join(GOLDEN, "poa_spans.json.gz"), "rt")))
    return _FX


def _members(seqs):
    return [(s.encode("latin-1"), None if q is None else q.encode("latin-1")) for s, q in seqs]


def _spans(spans):
    return [None if x is None else tuple(x) for x in spans]


def entries():
    """every entry of the fixture -> [(label, members as passed to the call, spans, algorithm, (m, n, g, e, q, c), strand, expected)]"""
    fx = load_spans_fixture()
    seeded = {g["name"]: g for g in fx["seeded"]}
    out = []
    for sec in ("seeded", "gaps", "strand", "hand"):
        for g in fx[sec]:
            src = seeded[g["name"]] if sec in ("gaps", "strand") else g
            mem, spans = _members(src["seqs"]), _spans(src["spans"])
            if sec == "strand":
                fl = set(g["flips"])
                mem = [(S.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(mem)]
            for t in ("0", "1", "2"):
                out.append((f"{sec}/{g['name']}/{g.get('model', 'linear')}/{t}", mem, spans, int(t), tuple(g["scores"]), sec == "strand",
                            g["expected"][t]))
            if "plain" in g:
                for t in ("0", "1", "2"):
                    out.append((f"{sec}/{g['name']}/plain/{t}", mem, [None] * len(mem), int(t), tuple(g["scores"]), False, g["plain"][t]))
    return out


def rows_digest(rows):
    return hashlib.sha256(b"\n".join(rows)).hexdigest()


def check_entry(got, e, label):
    """dict(consensus, rows, members, coverage, tables[, reversed, score, score_rev]) against a fixture entry"""
    assert got["consensus"].decode("latin-1") == e["consensus"], label
    assert list(got["coverage"]) == e["coverage"], label
    assert [m for m in got["members"] if m != pm.CONSENSUS] == e["members"], label
    rows = [bytes(r) for r in got["rows"]]
    assert (len(rows), len(rows[0]) if rows else 0) == (e["n_rows"], e["row_size"]), label
    if "rows" in e:
        assert rows == [r.encode("latin-1") for r in e["rows"]], label
    assert rows_digest(rows) == e["rows_sha256"], label
    t = got["tables"]
    assert G.counts(t) == e["counts"], (label, G.counts(t), e["counts"])
    if "tables" in e:
        want = G.unpack(e["tables"])
        for k in want:
            assert t[k] == want[k], (label, k)
    assert G.digest(t) == e["digest"], label
    if "reversed" in e:
        assert [int(x) for x in got["reversed"]] == e["reversed"], label
        assert [list(map(int, got["score"])), list(map(int, got["score_rev"]))] == [e["score"], e["score_rev"]], label


# ------------------------------------------------------------------ the boundary
def test_spans_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_spans" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_span_in" in hdr and "#define VC_POA_SPAN_NONE 0xFFFFFFFFu" in hdr
    assert "applies no span rule" in hdr and "Out of scope" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_spans")
    assert C.sizeof(capi.VcPoaSpanIn) == 16 and NONE == 0xFFFFFFFF
    assert len(capi.load_hip().vc_poa_run_spans.argtypes) == 7


def _raw(lib, groups, begin, end, p=None, null=()):
    """vc_poa_run_spans with the arrays as given -> (rc, message)"""
    batch = poa.group_batch(groups)
    cons, off, status, r, vb = poa._result_buffers(batch)
    sb, se = np.array(begin, np.uint32), np.array(end, np.uint32)
    ptr = lambda x, k: None if k in null else x.ctypes.data_as(C.POINTER(C.c_uint32))      # noqa: E731
    sp = capi.VcPoaSpanIn(ptr(sb, "begin"), ptr(se, "end"))
    rc = lib.vc_poa_run_spans(C.byref(p or _gp()), C.byref(sp), C.byref(vb), C.byref(r), None, None, None)
    return rc, lib.vc_poa_last_error().decode()


SPAN_ERRORS = [
    ("one_none_begin", [NONE, NONE, NONE, NONE, NONE], [NONE, NONE, NONE, NONE, 3], "member 1 of group 1", "only one"),
    ("one_none_end", [NONE, NONE, 2, NONE, NONE], [NONE, NONE, NONE, NONE, NONE], "member 2 of group 0", "only one"),
    ("begin_behind_end", [NONE, 5, NONE, NONE, NONE], [NONE, 4, NONE, NONE, NONE], "member 1 of group 0", "begins behind its end"),
    ("end_beyond_sequence_0", [NONE, NONE, NONE, NONE, 0], [NONE, NONE, NONE, NONE, 8], "member 1 of group 1", "ends beyond sequence 0"),
    ("first_violation_is_named", [NONE, 0, 9, NONE, 7], [NONE, 11, 3, NONE, 2], "member 2 of group 0", "begins behind its end"),
]


@pytest.mark.parametrize("case", SPAN_ERRORS, ids=[c[0] for c in SPAN_ERRORS])
def test_spans_are_refused_before_the_device(built, case):
    """no device is needed to be refused: every rule fires here, where there is none, with the group and the member named"""
    _, begin, end, who, what = case
    lib = capi.load_hip()
    groups = [[b"ACGTACGTACGT", b"ACGTAC", b"GTACGT"], [b"ACGTACGT", b"ACGT"]]
    rc, msg = _raw(lib, groups, begin, end)
    assert rc == capi.VC_ERR_ARG and who in msg and what in msg, (rc, msg)


def test_span_checks_come_after_the_batch_and_before_the_device(built):
    lib = capi.load_hip()
    groups = [[b"ACGTACGTACGT", b"ACGTAC"], [b"", b"ACGT"]]
    ok_b, ok_e = [NONE, 0, NONE, NONE], [NONE, 11, NONE, NONE]
    # the parameters first, then the span arrays, then the members
    rc, msg = _raw(lib, groups, [NONE, 5, NONE, NONE], [NONE, 4, NONE, NONE], p=_gp(algorithm=7))
    assert rc == capi.VC_ERR_ARG and "algorithm" in msg
    rc, msg = _raw(lib, groups, ok_b, ok_e, null=("end",))
    assert rc == capi.VC_ERR_ARG and "null span array" in msg
    # a group whose sequence 0 is empty admits no span; sequence 0's own entries are not read
    rc, msg = _raw(lib, groups, [NONE, NONE, NONE, 0], [NONE, NONE, NONE, 0])
    assert rc == capi.VC_ERR_ARG and "member 1 of group 1" in msg and "ends beyond sequence 0" in msg
    rc, msg = _raw(lib, groups, [77, 0, 9, NONE], [3, 11, NONE, NONE])
    if not _device_visible():
        assert rc == capi.VC_ERR_NO_DEVICE, (rc, msg)                   # valid spans: only the device is missing
        rc, msg = _raw(lib, groups, [NONE] * 4, [NONE] * 4)
        assert rc == capi.VC_ERR_NO_DEVICE


def test_python_validation(built):
    groups = [[b"ACGTACGTACGT", b"ACGTAC", b"GTACGT"], [b"ACGTACGT", (b"ACGT", b"IIII")]]
    assert poa.span_arrays(groups, None) is None
    assert poa.span_arrays(groups, [None, None]) is None
    assert poa.span_arrays(groups, [[None, None, None], [(3, 1), None]]) is None          # member 0's entry is not read
    b, e = poa.span_arrays(groups, [[None, (0, 5), None], [None, (4, 7)]])
    assert b.dtype == e.dtype == np.uint32
    assert b.tolist() == [NONE, 0, NONE, NONE, 4] and e.tolist() == [NONE, 5, NONE, NONE, 7]
    for bad, what in (([[None, (0, 5), None]], "span lists for 2 groups"), ([[None, None], None], "one entry per member"),
                      ([[None, (5, 4), None], None], "begin <= end"), ([[None, (-1, 4), None], None], "begin <= end"),
                      ([None, [None, (0, 8)]], "ends beyond sequence 0"), ([[None, (0, 12), None], None], "ends beyond sequence 0"),
                      ([[None, (0,), None], None], "pair of integers"), ([[None, (0, 2.5), None], None], "pair of integers"),
                      ([[None, "05", None], None], "pair of integers"), ([[None, (True, 2), None], None], "pair of integers")):
        with pytest.raises(ValueError, match=re.escape(what)):
            poa.span_arrays(groups, bad)
    sp = [[None, (0, 5), None], None]
    with pytest.raises(ValueError, match="takes no spans"):
        poa.poa_graph(groups, resumable=True, spans=sp)
    with pytest.raises(ValueError, match="takes no spans"):
        poa.poa_extend([None, None], groups, spans=sp)
    with pytest.raises(ValueError, match="takes no spans"):
        poa.poa_align(groups, [[b"ACGT"], [b"ACGT"]], spans=sp)
    with pytest.raises(ValueError, match="takes no spans"):
        poa.poa_correct(groups, spans=sp)
    with pytest.raises(ValueError, match="do not go with"):
        poa._run(poa.group_batch(groups), _gp(), spans=poa.span_arrays(groups, sp), state=True, graph=True)


def test_a_library_without_the_entry_says_rebuild(built):
    class Old:
        """a library from before the entry point"""
    groups = [[b"ACGTACGTACGT", b"ACGTAC"]]
    with pytest.raises(poa.PoaError, match="no vc_poa_run_spans.*rebuild"):
        poa.poa_consensus(groups, spans=[[None, (0, 5)]], lib=Old())


@pytest.mark.parametrize("L", [99, 100, 199, 200, 500])
def test_racon_spans_is_the_one_percent_rule(L):
    """window.cpp:207-208: offset = 0.01 * L as an integer; a layer spans when begin < offset and end > L - offset"""
    offset = L // 100
    assert offset == int(0.01 * L)
    pos = [None] + [(b, e) for b in range(0, offset + 3) for e in range(max(L - offset - 3, b), L)]
    got = poa.racon_spans(L, pos)
    assert len(got) == len(pos) and got[0] is None
    for p, g in zip(pos[1:], got[1:]):
        assert g == (None if p[0] < offset and p[1] > L - offset else p), (L, p, g)
    at = lambda p: got[1 + pos[1:].index(p)]                                                                  # noqa: E731
    if offset <= 1:
        # the end is inclusive, at most L - 1, and must exceed L - offset: below 200 bases no layer counts as spanning
        assert all(g is not None for g in got[1:]) and at((0, L - 1)) == (0, L - 1)
    else:
        assert at((0, L - 1)) is None and at((offset - 1, L - offset + 1)) is None
        assert at((offset, L - 1)) == (offset, L - 1) and at((0, L - offset)) == (0, L - offset)


def test_spans_parser():
    files = ["a.fasta", "dir/b.fastq"]
    records = [[("r0", b"ACGTACGT", None), ("r1", b"ACGT", None), ("r2", b"CGTA", None)], [("r0", b"ACGTAC", b"IIIIII"), ("x", b"GT", b"II")]]
    text = b"# group\tmember\tbegin\tend\na.fasta\tr2\t1\t4\n\ndir/b.fastq\tx\t2\t3\r\na.fasta\tr1\t0\t3\n"
    assert poa.parse_spans(text, files, records) == [[None, (0, 3), (1, 4)], [None, (2, 3)]]
    assert poa.parse_spans(b"", files, records) == [[None, None, None], [None, None]]
    for bad, what in ((b"c.fasta\tr1\t0\t3\n", "no input file named c.fasta"), (b"a.fasta\tx\t0\t3\n", "has no record named x"),
                      (b"a.fasta\tr1\t0\t3\na.fasta\tr1\t0\t3\n", "listed twice"), (b"a.fasta\tr1\t0\n", "separated by tabs"),
                      (b"a.fasta\tr1\t-1\t3\n", "separated by tabs"), (b"a.fasta r1 0 3\n", "separated by tabs")):
        with pytest.raises(ValueError, match=re.escape(what)):
            poa.parse_spans(bad, files, records)
    with pytest.raises(ValueError, match="more than one record named r0"):
        poa.parse_spans(b"a.fasta\tr0\t0\t3\n", ["a.fasta"], [[("r0", b"ACGT", None), ("r0", b"ACGT", None)]])
    with pytest.raises(ValueError, match="given twice"):
        poa.parse_spans(b"", ["a.fasta", "a.fasta"], [[], []])
    a = poa.parse_args(["--spans", "s.tsv", "a.fasta"])
    assert a.spans == "s.tsv" and poa.parse_args(["a.fasta"]).spans is None
    for other in (["--align", "q.fa", "--align-out", "o.tsv"], ["--correct", "c.fa"], ["--save-graphs", "g.npz"]):
        assert poa.main(["--spans", "s.tsv", *other, "a.fasta"]) == 1


# ------------------------------------------------------------------ the restatement against the reference
def _restate(a):
    label, mem, spans, t, scores, strand, e = a
    check_entry(SR.run(mem, spans, t, *scores, strands=strand), e, label)
    return label


def test_restatement_reproduces_every_fixture_entry():
    es = entries()
    assert len(es) == 111 and sum(1 for x in es if x[5]) == 15
    with ProcessPoolExecutor(_workers()) as ex:
        assert len(list(ex.map(_restate, es, chunksize=4))) == len(es)


def test_fixture_covers_what_it_claims():
    fx = load_spans_fixture()
    hand = {h["name"]: h for h in fx["hand"]}
    assert {"span_of_one_node", "spans_at_0_and_last", "member_longer_than_span", "member_shorter_than_span", "empty_member_with_span",
            "span_over_aligned_nodes", "two_members_same_span", "all_none", "repeat"} == set(hand)
    L = len(hand["spans_at_0_and_last"]["seqs"][0][0])
    sp = [tuple(x) for x in hand["spans_at_0_and_last"]["spans"][1:]]
    assert (0, 0) in sp and (L - 1, L - 1) in sp
    assert any(s == "" and x is not None for (s, _), x in zip(hand["empty_member_with_span"]["seqs"], hand["empty_member_with_span"]["spans"]))
    # the member that is longer than its span leaves new chains before and after: its path starts and ends on nodes of its own
    # (semi-global: a global alignment ends on the last node of the subgraph and puts the surplus inside)
    t = G.unpack(hand["member_longer_than_span"]["expected"]["2"]["tables"])
    L0 = len(hand["member_longer_than_span"]["seqs"][0][0])
    path = next(p for m, _, p in t["paths"] if m == 1)
    assert path[0] >= L0 and path[-1] >= L0 and any(v < L0 for v in path)
    # the aligned nodes that earlier mismatches left inside the later spans
    t = G.unpack(hand["span_over_aligned_nodes"]["expected"]["1"]["tables"])
    assert any(28 <= a <= 49 for a, _ in t["aligned"])
    assert len(fx["seeded"]) == 12 and len(fx["gaps"]) == 10 and len(fx["strand"]) == 5
    for g in fx["seeded"]:
        assert 60 <= len(g["seqs"][0][0]) <= 400 and 3 <= len(g["seqs"]) <= 24 and any(x is not None for x in g["spans"])
    assert any(q is not None for g in fx["seeded"] for _, q in g["seqs"])


def test_all_none_is_the_plain_flow():
    """no span at all: the plain restatement's bytes, and the consensus committed with the plain groups"""
    fx = load_spans_fixture()
    h = next(x for x in fx["hand"] if x["name"] == "all_none")
    src = next(g for g in load_fixture()["groups"] if g["name"] == "size3_len100_mixed")
    mem = _members(h["seqs"])
    assert h["seqs"] == src["seqs"] and all(x is None for x in h["spans"])
    for t in (0, 1, 2):
        got = SR.run(mem, h["spans"], t, *h["scores"])
        assert got["consensus"].decode() == src["expected"][str(t)]["consensus"] == h["expected"][str(t)]["consensus"]
        plain = pm.msa(mem, t, *h["scores"])
        assert (got["rows"], got["members"], got["consensus"], got["coverage"]) == (plain["rows"], plain["members"], plain["consensus"], plain["coverage"])
        assert got["tables"] == G.graph(mem, t, *h["scores"])
    g = fx["seeded"][3]                                                    # and on a group that has spans, with them taken away
    mem = _members(g["seqs"])
    assert SR.run(mem, None, 1, *g["scores"])["tables"] == G.graph(mem, 1, *g["scores"])
    assert SR.run(mem, _spans(g["spans"]), 1, *g["scores"])["tables"] != G.graph(mem, 1, *g["scores"])


def test_repeat_group_differs_from_the_plain_call_as_recorded():
    fx = load_spans_fixture()
    h = next(x for x in fx["hand"] if x["name"] == "repeat")
    mem, spans = _members(h["seqs"]), _spans(h["spans"])
    with_spans, plain = SR.run(mem, spans, 1, *h["scores"]), SR.run(mem, None, 1, *h["scores"])
    check_entry(with_spans, h["expected"]["1"], "repeat/spans")
    check_entry(plain, h["plain"]["1"], "repeat/plain")
    assert h["expected"]["1"]["digest"] != h["plain"]["1"]["digest"] and with_spans["rows"] != plain["rows"]
    # the plain global alignment starts the read on the first copy, which it spells, and stretches it to the backbone's end; the
    # span keeps it on the second copy, where it belongs
    on_backbone = lambda r: [v for v in next(p for m, _, p in r["tables"]["paths"] if m == 1) if v < len(mem[0][0])]      # noqa: E731
    assert on_backbone(plain)[:3] == [25, 26, 27] and on_backbone(plain)[-1] == len(mem[0][0]) - 1
    assert on_backbone(with_spans)[0] == 65 and on_backbone(with_spans)[-1] == 104


# ------------------------------------------------------------------ through the path the oracle already pins
def test_windows_through_the_span_flow_give_the_oracles_untrimmed_consensus(built):
    """Mode 1 of the oracle (the racon-linear overload, window.cpp:74-170) with trimming off is Subgraph / UpdateAlignment /
    AddAlignment over the rank-sorted layers and then the heaviest bundle: the span flow with racon_spans applied to the layers'
    positions, global, at the window's linear match / mismatch / gap.  Every window of tests/golden/windows.json with at least 3
    sequences qualifies -- the batch carries the layers in rank order already, a FASTA backbone with the dummy quality string that
    the window gives it (so the quality overload's weights agree), and no layer is empty; a window of fewer than 3 sequences is
    returned unpolished by a rule of the window (window.cpp:188-192) that a group does not have."""
    fx = fixtures.load_windows()
    batch = fixtures.fixture_batch(fx["windows"])
    p = capi.VcParams(**fx["params"])
    p.mode, p.trim = 1, 0
    cons, polished, _ = oa.oracle_run(batch, p)
    n = partial = 0
    for w in range(batch.n_windows):
        seqs, quals, b, e = batch.window(w)
        if len(seqs) < 3:
            assert not polished[w]
            continue
        s0 = int(batch.win_seq_off[w])
        mem = [(bytes(s), bytes(q) if batch.seq_has_qual[s0 + k] else None) for k, (s, q) in enumerate(zip(seqs, quals))]
        spans = poa.racon_spans(len(mem[0][0]), [None] + [(int(x), int(y)) for x, y in zip(b[1:], e[1:])])
        assert polished[w] and SR.run(mem, spans, 1, p.match, p.mismatch, p.gap)["consensus"] == cons[w], fx["windows"][w]["name"]
        n += 1
        partial += sum(1 for x in spans if x is not None)
    assert n == 23 and partial > 20
