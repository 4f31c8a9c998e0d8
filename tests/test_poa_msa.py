"""CPU suite: the multiple sequence alignment and coverage of POA groups (vc_poa_run_msa, poa.poa_msa, the command line's -r /
--coverage) at their boundary -- declared, exported and bound with the documented layout, the arguments refused before the device,
the parser -- and the CPU restatement tests/poa_msa_ref.py, the live bar for the device, against every entry of
tests/golden/poa_msa.json.gz (spoa's own output), with spoa's own invariants (test/spoa_test.cpp:54-76) on every entry."""
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
from poa_common import TYPES, _gp, _workers
from test_poa import _device_visible, load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_msa_fixture():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_msa.json.gz"), "rt"))


def entries():
    """every fixture entry -> [(label, members, algorithm, (m, n, g, e, q, c), expected)]"""
    fx = load_msa_fixture()
    seqs, quals = fixtures.load_sample_reads()
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    out = []
    for name, k in fx["kat"].items():
        out.append((name, list(zip(seqs, quals if k["quality"] else [None] * len(seqs))), TYPES[k["type"]], tuple(k["scores"]), k))
    for g in fx["groups"]:
        m, n, gp = g["scores"]
        for t in ("0", "1", "2"):
            out.append((f"{g['name']}/{t}", groups[g["name"]], int(t), (m, n, gp, gp, gp, gp), g["expected"][t]))
    for g in fx["gaps"]:
        for t in ("0", "1", "2"):
            out.append((f"{g['name']}/{g['model']}/{t}", groups[g["name"]], int(t), tuple(g["scores"]), g["expected"][t]))
    return out


# ------------------------------------------------------------------ the boundary
def test_msa_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_msa" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_msa_out" in hdr and "Lifetime" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_msa")
    # the documented field list: two uint32, five pointers, the rows pointer, its uint64 size, the coverage pointer
    assert [f for f, _ in capi.VcPoaMsaOut._fields_] == ["flags", "n_groups", "n_rows", "row_size", "row_off", "member_off",
                                                         "row_member", "rows", "rows_bytes", "coverage"]
    body = hdr[hdr.index("typedef struct vc_poa_msa_out"):hdr.index("} vc_poa_msa_out;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in capi.VcPoaMsaOut._fields_]
    assert C.sizeof(capi.VcPoaMsaOut) == 72 and capi.VcPoaMsaOut.rows.offset == 48 and capi.VcPoaMsaOut.coverage.offset == 64
    for name, v in (("VC_POA_MSA", 1), ("VC_POA_MSA_CONSENSUS", 2), ("VC_POA_COVERAGE", 4), ("VC_POA_ROW_CONSENSUS", 0xFFFFFFFF)):
        assert getattr(capi, name) == v
        assert int(re.search(rf"#define {name}\s+(\w+?)u\b", hdr).group(1), 0) == v
    assert C.sizeof(capi.VcPoaGapParams) == 32 and C.sizeof(capi.VcPoaParams) == 20      # unchanged


def _call(lib, params, batch, flags, out=True, **override):
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
    return lib.vc_poa_run_msa(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r), C.byref(o) if out else None)


def test_msa_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad = [("null params", lambda: _call(lib, None, b, 1)),
           ("null output description", lambda: _call(lib, _gp(), b, 1, out=False)),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b, 1)),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b, 1)),
           ("gap_extend2 > 0", lambda: _call(lib, _gp(gap_extend2=2), b, 1)),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b, 1)),
           ("unknown flag bit 8", lambda: _call(lib, _gp(), b, 8)),
           ("unknown flag bit 31", lambda: _call(lib, _gp(), b, 1 | (1 << 31))),
           ("consensus row without the MSA", lambda: _call(lib, _gp(), b, 2)),
           ("consensus row and coverage without the MSA", lambda: _call(lib, _gp(), b, 6)),
           ("null seq_off", lambda: _call(lib, _gp(), b, 7, seq_off=None)),
           ("null quals beside a quality", lambda: _call(lib, _gp(), b, 7, quals=None)),
           ("a sequence of 65 535 bases", lambda: _call(lib, _gp(), poa.group_batch([["A" * 65535]]), 1))]
    for what, f in bad:
        assert f() == capi.VC_ERR_ARG, what
        assert lib.vc_poa_last_error().decode(), what
    # vc_poa_run_gaps's order first, then the flags, then the batch
    assert _call(lib, _gp(match=500), b, 8) == capi.VC_ERR_ARG and "scores" in lib.vc_poa_last_error().decode()
    assert _call(lib, _gp(), b, 8, seq_off=None) == capi.VC_ERR_ARG and "flag" in lib.vc_poa_last_error().decode()


def test_valid_msa_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    for flags in (0, 1, 3, 4, 5, 7):
        for b in (poa.group_batch([["ACGT", ("ACGA", "IIII")], [], ["T"]]), poa.group_batch([])):
            assert _call(lib, _gp(), b, flags) == capi.VC_ERR_NO_DEVICE, flags
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_msa([["ACGT"]], "semi-global")
    assert ex.value.rc == capi.VC_ERR_NO_DEVICE and "vc_poa_run_msa" in str(ex.value)


class _Recorder:
    """stands in for the library: records the parameters and flags, returns every group empty and OK"""

    def __init__(self):
        self.calls = []

    def vc_poa_run_msa(self, p, b, r, o):
        self.calls.append(({f: getattr(p._obj, f) for f, _ in p._obj._fields_}, o._obj.flags))
        return 0

    def vc_poa_last_error(self):
        return b""


def test_poa_msa_parameters():
    lib = _Recorder()
    g = [["ACGT", "ACGA"], []]
    res = poa.poa_msa(g, lib=lib)
    assert [(m.rows, m.members, m.consensus, m.coverage) for m in res] == [([], [], b"", None)] * 2
    assert tuple(res[0]) == ([], [], b"", None)
    poa.poa_msa(g, "local", 3, -5, -4, 0, True, lib, include_consensus=True)
    res = poa.poa_msa(g, 2, gap=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4, coverage=True, lib=lib)
    assert res[0].coverage.dtype == np.uint32 and res[0].coverage.size == 0
    poa.poa_msa(g, include_consensus=True, coverage=True, lib=lib)
    assert [f for _, f in lib.calls] == [1, 3, 5, 7]
    assert lib.calls[0][0] == dict(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    assert lib.calls[1][0] == dict(device=0, algorithm=0, match=3, mismatch=-5, gap_open=-4, gap_extend=-4, gap_open2=-4, gap_extend2=-4)
    assert lib.calls[2][0] == dict(device=0, algorithm=2, match=5, mismatch=-4, gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4)
    with pytest.raises(TypeError):
        poa.poa_msa(g, "global", 5, -4, -8, 0, True, lib, True)           # keyword-only
    with pytest.raises(ValueError):
        poa.poa_msa([[("ACGT", "II")]], lib=lib)                          # a quality string of the wrong length
    with pytest.raises(ValueError):
        poa.poa_msa(g, "diagonal", lib=lib)
    with pytest.raises(TypeError):
        poa.poa_msa(["ACGT"], lib=lib)


def test_command_line_result_options(monkeypatch, tmp_path, capfdbinary):
    assert poa.parse_args(["x.fa"]).r == 0 and poa.parse_args(["x.fa"]).coverage is False
    a = poa.parse_args(["-r", "2", "-l", "1", "x.fa", "y.fa"])
    assert (a.r, a.l, a.files) == (2, 1, ["x.fa", "y.fa"])
    assert poa.parse_args(["-r1", "--coverage", "x.fa"]).coverage is True
    for argv in (["-r", "3", "x.fa"], ["-r", "4", "x.fa"], ["-r", "-1", "x.fa"], ["-r", "x.fa"], ["--dot", "g.dot", "x.fa"],
                 ["--strand-ambiguous", "x.fa"], ["-s", "x.fa"], ["-d", "g.dot", "x.fa"]):
        with pytest.raises(SystemExit):
            poa.parse_args(argv)
    capfdbinary.readouterr()
    fa, fb = tmp_path / "x.fa", tmp_path / "y.fq"
    fa.write_text(">r1\nACGT\n>r2\n\n>r3\nACT\n")
    fb.write_text("@q1\nGG\n+\nII\n")
    got = []

    def fake(groups, *args, **kw):
        got.append((args, kw))
        c = poa.CONSENSUS_ROW
        return [poa.Msa([b"ACGT", b"AC-T"] + ([b"ACGT"] if kw["include_consensus"] else []), [0, 2] + ([c] if kw["include_consensus"] else []),
                        b"ACGT", np.array([2, 2, 1, 2], np.uint32) if kw["coverage"] else None),
                poa.Msa([b"GG"] + ([b"GG"] if kw["include_consensus"] else []), [0] + ([c] if kw["include_consensus"] else []), b"GG",
                        np.array([0, 0], np.uint32) if kw["coverage"] else None)][:len(groups)]
    monkeypatch.setattr(poa, "poa_msa", fake)
    monkeypatch.setattr(poa, "poa_consensus", lambda *a, **k: pytest.fail("-r 1 must not take the consensus-only path"))
    assert poa.main(["-r", "1", "-l", "2", str(fa), str(fb)]) == 0
    assert capfdbinary.readouterr().out == b">r1\nACGT\n>r3\nAC-T\n>q1\nGG\n"          # the empty record r2 has no row
    assert got[0][0] == (2, 5, -4, -8) and got[0][1]["include_consensus"] is False and got[0][1]["coverage"] is False
    assert poa.main(["-r", "2", str(fa), str(fb)]) == 0
    assert capfdbinary.readouterr().out == b">r1\nACGT\n>r3\nAC-T\n>Consensus\nACGT\n>q1\nGG\n>Consensus\nGG\n"
    assert poa.main(["--coverage", str(fa), str(fb)]) == 0
    assert capfdbinary.readouterr().out == b">Consensus LN:i:4 CV:B:I,2,2,1,2\nACGT\n>Consensus LN:i:2 CV:B:I,0,0\nGG\n"
    assert poa.main(["-r", "1", "--coverage", str(fa)]) == 1
    assert b"--coverage" in capfdbinary.readouterr().err
    for word in ("-r 1", "-r 2", "CV:B:I", "GFA", "--dot", "--strand-ambiguous", "poa_msa"):
        assert word in poa.__doc__, word


# ------------------------------------------------------------------ the fixture and the restatement
def test_fixture_shape():
    fx = load_msa_fixture()
    assert len(fx["kat"]) == 18 and set(fx["kat"]) == set(json.load(open(os.path.join(GOLDEN, "spoa_kat_gaps.json"))))
    assert [g["name"] for g in fx["groups"]] == [g["name"] for g in load_fixture()["groups"]]
    assert {g["model"] for g in fx["gaps"]} == {"affine", "convex"} and any(g["name"] == "empty_sequence_between" for g in fx["gaps"])
    assert os.path.getsize(os.path.join(GOLDEN, "poa_msa.json.gz")) < (1 << 20)
    # the consensus entries are the committed ones: the same run
    kats = json.load(open(os.path.join(GOLDEN, "spoa_kat_gaps.json")))
    for name, k in fx["kat"].items():
        assert k["consensus"] == kats[name]["consensus"], name
    for g, h in zip(fx["groups"], load_fixture()["groups"]):
        for t in ("0", "1", "2"):
            assert g["expected"][t]["consensus"] == h["expected"][t]["consensus"], (g["name"], t)


def test_spoas_invariants_hold_on_every_fixture_entry():
    n = 0
    for label, mem, t, scores, e in entries():
        rows = [r.encode() for r in e["rows"]]
        M.check_invariants(rows, e["members"] + [M.CONSENSUS], mem, True)
        assert rows[-1].replace(b"-", b"").decode() == e["consensus"], label
        assert len(e["coverage"]) == len(e["consensus"]), label
        M.check_invariants(rows[:-1], e["members"], mem, False)
        n += 1
    assert n == 18 + 3 * 30 + 3 * 10
    es = {l: e for l, _, _, _, e in entries()}
    assert es["empty_group/1"]["rows"] == [""] and es["empty_sequences_only/1"]["rows"] == [""]      # one consensus row of length 0
    assert es["empty_sequence_first/1"]["members"] == [1, 2, 3, 4]


def _job(i):
    label, mem, t, scores, e = entries()[i]
    got = M.msa(mem, t, *scores, include_consensus=True)
    return label, (got["rows"] == [r.encode() for r in e["rows"]], got["members"] == e["members"] + [M.CONSENSUS],
                   got["consensus"].decode() == e["consensus"], got["coverage"] == e["coverage"])


def test_restatement_reproduces_every_fixture_entry():
    es = entries()
    order = sorted(range(len(es)), key=lambda i: -len(es[i][1]) * sum(len(s) for s, _ in es[i][1]))
    with ProcessPoolExecutor(_workers()) as ex:
        for label, ok in ex.map(_job, order):
            assert ok == (True, True, True, True), (label, ok)


def test_restatement_without_the_consensus_row():
    mem = [(b"ACGTACGT", None), (b"", None), (b"ACGAACGT", b"IIIIIIII"), (b"CGTAC", None)]
    a, b = M.msa(mem, 1, 5, -4, -8, include_consensus=False), M.msa(mem, 1, 5, -4, -8, include_consensus=True)
    assert a["rows"] == b["rows"][:-1] and a["members"] == [0, 2, 3] and b["members"] == [0, 2, 3, M.CONSENSUS]
    M.check_invariants(a["rows"], a["members"], mem, False)
    assert len(a["coverage"]) == len(a["consensus"]) and max(a["coverage"]) <= 3
