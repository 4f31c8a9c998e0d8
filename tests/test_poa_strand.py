"""CPU suite: strand-ambiguous POA groups (vc_poa_run_strand, poa.poa_consensus_strands, poa.poa_msa(strand_ambiguous=True),
the command line's --both-strands) at their boundary -- declared, exported and bound with the documented layout, the arguments
refused before the device, the parser -- and the CPU restatement tests/poa_strand_ref.py, the live bar for the device, against
every entry of tests/golden/poa_strand.json.gz (spoa's own output)."""
import ctypes as C
import gzip
import json
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import poa_msa_ref as M
import poa_strand_ref as S
from poa_common import TYPES, _gp, _workers
from test_poa import _device_visible, load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_strand_fixture():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_strand.json.gz"), "rt"))


def flipped(mem, flips):
    """the members named in `flips` reverse-complemented, their quality strings reversed"""
    fl = set(flips)
    return [(S.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(mem)]


def entries():
    """every fixture entry -> [(label, members as passed to the call, algorithm, (m, n, g, e, q, c), expected)]"""
    fx = load_strand_fixture()
    seqs, quals = fixtures.load_sample_reads()
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    out = []
    for name, k in fx["kat"].items():
        mem = flipped(list(zip(seqs, quals if k["quality"] else [None] * len(seqs))), k["flips"])
        out.append((name, mem, TYPES[k["type"]], tuple(k["scores"]), k))
    for g in fx["groups"]:
        m, n, gp = g["scores"]
        for t in ("0", "1", "2"):
            out.append((f"{g['name']}/{t}", flipped(groups[g["name"]], g["flips"]), int(t), (m, n, gp, gp, gp, gp), g["expected"][t]))
    for g in fx["gaps"]:
        for t in ("0", "1", "2"):
            out.append((f"{g['name']}/{g['model']}/{t}", flipped(groups[g["name"]], g["flips"]), int(t), tuple(g["scores"]),
                        g["expected"][t]))
    for g in fx["hand"]:
        sc = tuple(g["scores"]) if len(g["scores"]) == 6 else (g["scores"][0], g["scores"][1]) + (g["scores"][2],) * 4
        for t in ("0", "1", "2"):
            out.append((f"hand/{g['name']}/{t}", members(g), int(t), sc, g["expected"][t]))
    return out


# ------------------------------------------------------------------ the boundary
def test_strand_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_strand" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_strand_out" in hdr and "round-trip rule" in hdr and "tie rule" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_strand")
    assert [f for f, _ in capi.VcPoaStrandOut._fields_] == ["reversed", "score", "score_rev"]
    body = hdr[hdr.index("typedef struct vc_poa_strand_out"):hdr.index("} vc_poa_strand_out;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in capi.VcPoaStrandOut._fields_]
    assert C.sizeof(capi.VcPoaStrandOut) == 24 and capi.VcPoaStrandOut.score.offset == 8 and capi.VcPoaStrandOut.score_rev.offset == 16
    assert capi.load_hip().vc_poa_run_strand.argtypes[3:] == [C.POINTER(capi.VcPoaMsaOut), C.POINTER(capi.VcPoaStrandOut)]
    assert C.sizeof(capi.VcPoaMsaOut) == 72 and C.sizeof(capi.VcPoaGapParams) == 32                      # unchanged


def _call(lib, params, batch, flags, out=True, strand="all", **override):
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in override.items():
        setattr(vb, k, v)
    o = capi.VcPoaMsaOut(flags=flags)
    n = max(int(batch.win_seq_off[-1]) if batch.n_windows else 0, 1)
    rev, sc, scr = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    s = capi.VcPoaStrandOut()
    if strand in ("all", "flags only"):
        s.reversed = rev.ctypes.data_as(C.POINTER(C.c_uint8))
    if strand == "all":
        s.score, s.score_rev = sc.ctypes.data_as(C.POINTER(C.c_int32)), scr.ctypes.data_as(C.POINTER(C.c_int32))
    return lib.vc_poa_run_strand(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r), C.byref(o) if out else None,
                                 C.byref(s) if strand != "null" else None)


def test_strand_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad = [("null params", lambda: _call(lib, None, b, 1)),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b, 1)),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b, 1)),
           ("gap_extend2 > 0", lambda: _call(lib, _gp(gap_extend2=2), b, 1)),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b, 1)),
           ("unknown flag bit 8", lambda: _call(lib, _gp(), b, 8)),
           ("consensus row without the MSA", lambda: _call(lib, _gp(), b, 2)),
           ("null strand output", lambda: _call(lib, _gp(), b, 1, strand="null")),
           ("null strand output, consensus only", lambda: _call(lib, _gp(), b, 0, out=False, strand="null")),
           ("null reversed array", lambda: _call(lib, _gp(), b, 1, strand="no arrays")),
           ("null seq_off", lambda: _call(lib, _gp(), b, 7, seq_off=None)),
           ("null quals beside a quality", lambda: _call(lib, _gp(), b, 7, quals=None)),
           ("a sequence of 65 535 bases", lambda: _call(lib, _gp(), poa.group_batch([["A" * 65535]]), 1))]
    for what, f in bad:
        assert f() == capi.VC_ERR_ARG, what
        assert lib.vc_poa_last_error().decode(), what
    # vc_poa_run_msa's order first (scores, then flags), then the strand output, then the batch
    assert _call(lib, _gp(match=500), b, 8, strand="null") == capi.VC_ERR_ARG and "scores" in lib.vc_poa_last_error().decode()
    assert _call(lib, _gp(), b, 8, strand="null") == capi.VC_ERR_ARG and "flag" in lib.vc_poa_last_error().decode()
    assert _call(lib, _gp(), b, 1, strand="null", seq_off=None) == capi.VC_ERR_ARG and "strand" in lib.vc_poa_last_error().decode()
    assert _call(lib, _gp(), b, 1, seq_off=None) == capi.VC_ERR_ARG and "batch" in lib.vc_poa_last_error().decode()


def test_valid_strand_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    for b in (poa.group_batch([["ACGT", ("ACGA", "IIII")], [], ["T"]]), poa.group_batch([])):
        for flags in (0, 1, 3, 4, 5, 7):
            assert _call(lib, _gp(), b, flags) == capi.VC_ERR_NO_DEVICE, flags
        assert _call(lib, _gp(), b, 0, out=False) == capi.VC_ERR_NO_DEVICE                    # o == NULL: the consensus only
        assert _call(lib, _gp(), b, 1, strand="flags only") == capi.VC_ERR_NO_DEVICE           # the scores are optional
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_consensus_strands([["ACGT"]], "semi-global")
    assert ex.value.rc == capi.VC_ERR_NO_DEVICE and "vc_poa_run_strand" in str(ex.value)
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_msa([["ACGT"]], strand_ambiguous=True)
    assert "vc_poa_run_strand" in str(ex.value)


class _Recorder:
    """stands in for the library: records the entry, the parameters and the flags; returns every group empty and OK and marks
    every second sequence of the batch reversed, with scores 2 i and 2 i + 1"""

    def __init__(self):
        self.calls = []

    def vc_poa_run_msa(self, p, b, r, o):
        self.calls.append(("msa", {f: getattr(p._obj, f) for f, _ in p._obj._fields_}, o._obj.flags))
        return 0

    def vc_poa_run_strand(self, p, b, r, o, s):
        self.calls.append(("strand", {f: getattr(p._obj, f) for f, _ in p._obj._fields_}, o._obj.flags))
        vb = b._obj
        for i in range(vb.win_seq_off[vb.n_windows]):
            s._obj.reversed[i], s._obj.score[i], s._obj.score_rev[i] = i & 1, 2 * i, 2 * i + 1
        return 0

    def vc_poa_last_error(self):
        return b""


def test_python_parameters():
    lib = _Recorder()
    g = [["ACGT", "ACGA", ""], [], ["TT", ("AC", "II")]]
    cons, rev = poa.poa_consensus_strands(g, lib=lib)
    assert cons == [b"", b"", b""]
    assert [r.dtype for r in rev] == [np.dtype(bool)] * 3 and [r.tolist() for r in rev] == [[False, True, False], [], [True, False]]
    cons, rev, sc, scr = poa.poa_consensus_strands(g, "local", 3, -5, -4, 0, True, lib, gap_extend=-2, gap_open2=-6, gap_extend2=-1,
                                                   scores=True)
    assert [x.dtype for x in sc + scr] == [np.dtype(np.int32)] * 6
    assert [x.tolist() for x in sc] == [[0, 2, 4], [], [6, 8]] and [x.tolist() for x in scr] == [[1, 3, 5], [], [7, 9]]
    res = poa.poa_msa(g, 2, include_consensus=True, coverage=True, strand_ambiguous=True, lib=lib)
    assert [m.reversed.tolist() for m in res] == [[False, True, False], [], [True, False]]
    assert tuple(res[0]) == ([], [], b"", res[0].coverage)                                  # __iter__ keeps its four
    plain = poa.poa_msa(g, lib=lib)
    assert plain[0].reversed is None and poa.Msa([], [], b"", None).reversed is None
    assert [(c[0], c[2]) for c in lib.calls] == [("strand", 0), ("strand", 0), ("strand", 7), ("msa", 1)]
    assert lib.calls[0][1] == dict(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    assert lib.calls[1][1] == dict(device=0, algorithm=0, match=3, mismatch=-5, gap_open=-4, gap_extend=-2, gap_open2=-6, gap_extend2=-1)
    assert lib.calls[2][1]["algorithm"] == 2
    with pytest.raises(TypeError):
        poa.poa_consensus_strands(g, "global", 5, -4, -8, 0, True, lib, -6)                 # keyword-only
    with pytest.raises(TypeError):
        poa.poa_msa(g, "global", 5, -4, -8, 0, True, lib, None, None, None, False, False, True)
    with pytest.raises(ValueError):
        poa.poa_consensus_strands([[("ACGT", "II")]], lib=lib)
    with pytest.raises(ValueError):
        poa.poa_consensus_strands(g, "diagonal", lib=lib)


def test_command_line_both_strands(monkeypatch, tmp_path, capfdbinary):
    assert poa.parse_args(["x.fa"]).both_strands is False
    for argv in (["--both-strands", "x.fa"], ["-r", "1", "--both-strands", "x.fa"], ["-r2", "--both-strands", "x.fa"],
                 ["--coverage", "--both-strands", "-l", "2", "x.fa"]):
        assert poa.parse_args(argv).both_strands is True
    fa = tmp_path / "x.fa"
    fa.write_text(">r1\nACGT\n>r2\nACT\n")
    got = []

    def fake_msa(groups, *args, **kw):
        got.append(("msa", groups, args, kw))
        return [poa.Msa([b"ACGT", b"AC-T"], [0, 1], b"ACGT", np.array([2, 2, 1, 2], np.uint32), np.array([False, True]))]

    def fake_strands(groups, *args, **kw):
        got.append(("strands", groups, args, kw))
        return [b"ACGT"], [np.array([False, True])]
    monkeypatch.setattr(poa, "poa_msa", fake_msa)
    monkeypatch.setattr(poa, "poa_consensus_strands", fake_strands)
    monkeypatch.setattr(poa, "poa_consensus", lambda *a, **k: pytest.fail("--both-strands must not take the plain path"))
    assert poa.main(["--both-strands", "-l", "1", str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">Consensus LN:i:4\nACGT\n"
    assert got[-1][0] == "strands" and got[-1][2] == (1, 5, -4, -8) and got[-1][1] == [[(b"ACGT", None), (b"ACT", None)]]
    assert poa.main(["--both-strands", "-r", "1", str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">r1\nACGT\n>r2\nAC-T\n"                      # the format says nothing about strands
    assert got[-1][0] == "msa" and got[-1][3]["strand_ambiguous"] is True
    assert poa.main(["--both-strands", "--coverage", str(fa)]) == 0
    assert capfdbinary.readouterr().out == b">Consensus LN:i:4 CV:B:I,2,2,1,2\nACGT\n"
    assert got[-1][3]["strand_ambiguous"] is True and got[-1][3]["coverage"] is True
    assert poa.main(["-r", "1", str(fa)]) == 0 and "strand_ambiguous" not in got[-1][3]
    capfdbinary.readouterr()
    for word in ("--both-strands", "GFA", "--dot", "--strand-ambiguous", "poa_consensus_strands", "only U"):
        assert word in poa.__doc__, word


# ------------------------------------------------------------------ the complement
def test_complement_and_round_trip_over_all_bytes():
    pairs = {"A": "T", "T": "A", "C": "G", "G": "C", "U": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H",
             "H": "D"}
    for c in range(256):
        ch = chr(c)
        want = ord(pairs[ch.upper()]) if ch.upper() in pairs and c < 128 else c
        assert S.COMPLEMENT[c] == want, c
        assert S.complement_byte(c) == want
    changed = {c for c in range(256) if S.ROUND_TRIP[c] != c}
    assert changed == {ord(x) for x in "acgtrykmbdhvuU"}
    assert S.ROUND_TRIP[ord("u")] == S.ROUND_TRIP[ord("U")] == ord("T")
    for x in "acgtrykmbdhv":
        assert S.ROUND_TRIP[ord(x)] == ord(x.upper())
    for x in "swnSWN-*.xX":
        assert S.COMPLEMENT[ord(x)] == ord(x) == S.ROUND_TRIP[ord(x)]
    assert S.reverse_complement(b"AACGTun") == b"nAACGTT" and S.round_trip(b"acgUusN") == b"ACGTTsN"
    assert S.kept_view(b"ACg", b"!#I", True) == (b"CGT", b"I#!") and S.kept_view(b"ACg", b"!#I", False) == (b"ACG", b"!#I")
    assert S.reverse_complement(b"ACGT" * 3) == b"ACGT" * 3


# ------------------------------------------------------------------ the fixture and the restatement
def test_fixture_shape_and_conditions():
    fx = load_strand_fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "poa_strand.json.gz")) < (1 << 20)
    assert len(fx["kat"]) == 18 and set(fx["kat"]) == set(json.load(open(os.path.join(GOLDEN, "spoa_kat_gaps.json"))))
    assert all(k["flips"] == list(range(1, 55, 2)) for k in fx["kat"].values())
    assert [g["name"] for g in fx["groups"]] == [g["name"] for g in load_fixture()["groups"]]
    assert sum(1 for g in fx["groups"] if 0 in g["flips"]) >= 5 and sum(1 for g in fx["groups"] if g["flips"] and 0 not in g["flips"]) >= 5
    assert {g["model"] for g in fx["gaps"]} == {"affine", "convex"} and len(fx["gaps"]) == 10
    names = {g["name"] for g in fx["hand"]}
    assert {"round_trip_kept_and_reversed", "reverse_palindrome_tie", "local_nothing_on_either_strand", "local_only_in_reverse",
            "empty_members_between", "single_member", "empty_group"} <= names
    es = entries()
    assert len(es) == 18 + 3 * 30 + 3 * 10 + 3 * len(fx["hand"])
    for label, mem, t, scores, e in es:
        assert len(e["reversed"]) == len(e["score"]) == len(e["score_rev"]) == len(mem), label
        assert e["members"] == [i for i, (s, _) in enumerate(mem) if len(s)], label
        assert len(e["rows"]) == len(e["members"]) + 1 and len(e["coverage"]) == len(e["consensus"]), label
        for i, (s, q) in enumerate(mem):
            assert e["reversed"][i] == (0 if e["score"][i] >= e["score_rev"][i] else 1), (label, i)     # ties go forward
            if not len(s):
                assert (e["reversed"][i], e["score"][i], e["score_rev"][i]) == (0, 0, 0), (label, i)
        first = next((i for i, (s, _) in enumerate(mem) if len(s)), None)
        if first is not None:                                                                          # it meets the empty graph
            assert (e["reversed"][first], e["score"][first], e["score_rev"][first]) == (0, 0, 0), label
        # a row without its gaps is the kept view of its member
        for row, i in zip(e["rows"], e["members"]):
            assert row.replace("-", "").encode() == S.kept_view(mem[i][0], mem[i][1], e["reversed"][i])[0], (label, i)
        assert e["rows"][-1].replace("-", "") == e["consensus"], label
    # the conditions that keep the fixture from proving nothing
    assert 2 * sum(1 for *_, e in es if any(e["reversed"])) >= len(es)
    assert any(a == b != 0 for *_, e in es for a, b in zip(e["score"], e["score_rev"]))
    assert any(not r and S.round_trip(s) != s for _, mem, _, _, e in es for (s, _), r in zip(mem, e["reversed"]))
    assert all(e["plain_agrees"] for *_, e in es if not e["round_trip_changes"])
    by = {l: e for l, _, _, _, e in es}
    assert by["hand/local_nothing_on_either_strand/0"]["score"][:2] == [0, 0] == by["hand/local_nothing_on_either_strand/0"]["score_rev"][:2]
    assert by["hand/local_only_in_reverse/0"]["reversed"][1] == 1 and by["hand/local_only_in_reverse/0"]["score"][1] == 0
    assert not any(by["hand/reverse_palindrome_tie/1"]["reversed"]) and by["hand/reverse_palindrome_tie/1"]["score"][1] == 200
    # with upper-case ACGT members a flip list that holds member 0 turns the whole group: reversed == flip XOR flip[0]
    for g in fx["groups"]:
        if g["name"].startswith("size17_len"):
            fl = [int(i in g["flips"]) for i in range(17)]
            assert g["expected"]["1"]["reversed"] == [f ^ fl[0] for f in fl], g["name"]


def _job(i):
    label, mem, t, scores, e = entries()[i]
    got = S.strands(mem, t, *scores, include_consensus=True)
    return label, ([int(r) for r in got["reversed"]] == e["reversed"], got["score"] == e["score"], got["score_rev"] == e["score_rev"],
                   got["rows"] == [r.encode() for r in e["rows"]], got["members"] == e["members"] + [M.CONSENSUS],
                   got["consensus"].decode() == e["consensus"], got["coverage"] == e["coverage"])


def test_restatement_reproduces_every_fixture_entry():
    es = entries()
    order = sorted(range(len(es)), key=lambda i: -len(es[i][1]) * sum(len(s) for s, _ in es[i][1]))
    with ProcessPoolExecutor(_workers()) as ex:
        for label, ok in ex.map(_job, order):
            assert ok == (True,) * 7, (label, ok)
