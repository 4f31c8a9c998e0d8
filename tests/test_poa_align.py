"""CPU suite: queries against finished POA groups (vc_poa_run_align, poa.poa_align, the command line's --align) at the boundary
-- declared, exported and bound with the documented layout, the arguments refused before the device in the documented order,
the Python checks, the TSV writer -- and the CPU restatement tests/poa_align_ref.py, the live bar for the device, against every
entry of tests/golden/poa_align.json.gz (spoa's own Align on the finished graph)."""
import ctypes as C
import gzip
import json
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import poa_align_ref as A
from poa_strand_ref import reverse_complement
from poa_common import TYPES, _gp, _workers
from test_poa import _device_visible, load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_FX = {}


def load_align_fixture():
    if not _FX:
        _FX.update(json.load(gzip.open(os.path.join(GOLDEN, "poa_align.json.gz"), "rt")))
    return _FX


def entries():
    """every entry of the fixture -> [(label, members, queries of the plain run, queries of the strand run, algorithm,
    (m, n, g, e, q, c), expected {"plain": [...], "strand": [...]})]"""
    fx = load_align_fixture()
    seqs, quals = fixtures.load_sample_reads()
    groups = {g["name"]: members(g) for g in load_fixture()["groups"]}
    out = []

    def add(label, mem, queries, flips, t, scores, e):
        fl = set(flips)
        out.append((label, mem, queries, [reverse_complement(s) if i in fl else s for i, s in enumerate(queries)], t, scores, e))
    for name, k in fx["kat"].items():
        add(f"kat/{name}", list(zip(seqs[:40], quals[:40] if k["quality"] else [None] * 40)), list(seqs[40:]), k["flips"], TYPES[k["type"]],
            tuple(k["scores"]), k)
    for sec in ("groups", "gaps", "hand"):
        for g in fx[sec]:
            mem = members(g) if sec == "hand" else groups[g["name"]]
            sc = tuple(g["scores"]) if len(g["scores"]) == 6 else (g["scores"][0], g["scores"][1]) + (g["scores"][2],) * 4
            queries = [s.encode("latin-1") for s in g["queries"]]
            for t in ("0", "1", "2"):
                add(f"{sec}/{g['name']}/{g.get('model', 'linear')}/{t}", mem, queries, g["flips"], int(t), sc, g["expected"][t])
    return out


# ------------------------------------------------------------------ the boundary
def test_align_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_align" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "#define VC_POA_ALIGN_PAIRS    1u" in hdr and "#define VC_POA_ALIGN_STRANDS  2u" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_align")
    body = hdr[hdr.index("typedef struct vc_poa_align_out"):hdr.index("} vc_poa_align_out;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in capi.VcPoaAlignOut._fields_]
    assert C.sizeof(capi.VcPoaAlignOut) == 80 and capi.VcPoaAlignOut.n_queries.offset == 8 and capi.VcPoaAlignOut.bytes.offset == 72
    assert capi.load_hip().vc_poa_run_align.argtypes[3:] == [C.POINTER(capi.VcPoaStrandOut), C.POINTER(capi.VcPoaGraphOut),
                                                             C.POINTER(capi.VcBatch), C.POINTER(capi.VcPoaAlignOut)]
    assert (capi.VC_POA_ALIGN_PAIRS, capi.VC_POA_ALIGN_STRANDS) == (1, 2)
    assert C.sizeof(capi.VcPoaGraphOut) == 152 and C.sizeof(capi.VcPoaMsaOut) == 72 and C.sizeof(capi.VcPoaStrandOut) == 24   # unchanged


def _call(lib, params, batch, qbatch, flags=1, out=True, strand="none", graph=False, queries=True, boverride=None, **qoverride):
    """-> (rc, the library's message, the align output)"""
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in (boverride or {}).items():
        setattr(vb, k, v)
    qv = qbatch.as_struct()
    qv.seq_begin = qv.seq_end = qv.win_fasta = qv.seq_has_qual = qv.quals = None
    for k, v in qoverride.items():
        setattr(qv, k, v)
    rev = np.zeros(max(int(batch.win_seq_off[-1]) if batch.n_windows else 0, 1), np.uint8)
    s = capi.VcPoaStrandOut()
    if strand == "all":
        s.reversed = rev.ctypes.data_as(C.POINTER(C.c_uint8))
    g = capi.VcPoaGraphOut()
    a = capi.VcPoaAlignOut(flags=flags)
    a.status = C.cast(1, C.POINTER(C.c_uint8))                                  # a failed call must leave every pointer NULL
    rc = lib.vc_poa_run_align(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r), C.byref(s) if strand != "none" else None,
                              C.byref(g) if graph else None, C.byref(qv) if queries else None, C.byref(a) if out else None)
    return rc, lib.vc_poa_last_error().decode(), a


def test_align_argument_errors_come_before_the_device_in_the_documented_order(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    q = poa.query_batch([["ACG"], ["AC", ""]])
    long_q = capi.Batch(np.array([0, 1, 1], np.uint32), np.array([0, 65535], np.uint64), [0], [0], [0], np.zeros(65535, np.uint8) + 65,
                        np.zeros(65535, np.uint8), np.zeros(2, np.uint8))
    three = poa.query_batch([["A"], ["C"], ["G"]])
    dec = (C.c_uint64 * 4)(0, 3, 2, 5)
    # one defect each, in the documented order: 1 as vc_poa_run_graph (the batch included), 2 the output and its flags, 3 the query
    # batch and its count, 4 the query lengths
    bad = [("null params", lambda: _call(lib, None, b, q), "null argument"),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b, q), "algorithm"),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b, q), "opening"),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b, q), "-128..127"),
           ("strand output without reversed", lambda: _call(lib, _gp(), b, q, strand="null"), "strand"),
           ("batch offsets decrease", lambda: _call(lib, _gp(), b, q, boverride=dict(seq_off=dec)), "seq_off decreases"),
           ("null align output", lambda: _call(lib, _gp(), b, q, out=False), "null align output"),
           ("unknown flag bit 4", lambda: _call(lib, _gp(), b, q, flags=4), "unknown align flag"),
           ("null query batch", lambda: _call(lib, _gp(), b, q, queries=False), "null query batch"),
           ("query count differs", lambda: _call(lib, _gp(), b, three), "one window per group"),
           ("query offsets decrease", lambda: _call(lib, _gp(), b, q, seq_off=dec), "query batch decreases"),
           ("null query bases", lambda: _call(lib, _gp(), b, q, bases=None), "null bases in the query batch"),
           ("query of 65 535 bases", lambda: _call(lib, _gp(), b, long_q), "query length")]
    for what, f, msg in bad:
        rc, text, a = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (what, rc, text)
        assert what == "null align output" or (not a.status and not a.score and not a.pair_off), what   # (that call passes no output)
    # two defects: the earlier check answers
    order = [(lambda: _call(lib, _gp(algorithm=3), b, q, out=False), "algorithm"),
             (lambda: _call(lib, _gp(), b, q, out=False, boverride=dict(seq_off=dec)), "seq_off decreases"),
             (lambda: _call(lib, _gp(), b, q, out=False, queries=False), "null align output"),
             (lambda: _call(lib, _gp(), b, three, flags=8), "unknown align flag"),
             (lambda: _call(lib, _gp(), b, q, flags=8, queries=False), "unknown align flag"),
             (lambda: _call(lib, _gp(), b, long_q, queries=False), "null query batch")]
    for f, msg in order:
        rc, text, _ = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (msg, rc, text)
    if not _device_visible():                                                   # valid arguments reach the device check, and only then
        for kw in (dict(), dict(graph=True), dict(strand="all"), dict(flags=3), dict(flags=0)):
            rc, text, a = _call(lib, _gp(), b, q, **kw)
            assert rc == capi.VC_ERR_NO_DEVICE and not a.status, (kw, rc, text)


def test_poa_align_raises_on_mismatched_counts():
    with pytest.raises(ValueError, match="1 query lists for 2 groups"):
        poa.poa_align([["ACGT"], ["AC"]], [["AC"]])
    with pytest.raises(TypeError):
        poa.poa_align([["ACGT"]], [[5]])
    qb = poa.query_batch([["ACG", b"T"], [], [""]])
    assert qb.win_seq_off.tolist() == [0, 2, 2, 3] and qb.seq_off.tolist() == [0, 3, 4, 4] and qb.bases.tobytes() == b"ACGT"


def test_command_line_options_for_align(capsys):
    a = poa.parse_args(["--align", "q.fa", "--align-out", "o.tsv", "--align-both-strands", "g.fa"])
    assert (a.align, a.align_out, a.align_both_strands, a.files) == ("q.fa", "o.tsv", True, ["g.fa"])
    assert poa.main(["--align", "q.fa", "g.fa"]) == 1 and "go together" in capsys.readouterr().err
    assert poa.main(["--align-both-strands", "g.fa"]) == 1


def test_tsv_writer_on_a_fixture_entry():
    """hand/local_finds_nothing, local alignment, linear gaps: the group is A x 20 and A x 19; CCCCCCCCCC and GGGGG find nothing,
    AAAA matches the first four nodes.  Beside it a second 'group' with hand-made results: both kinds of -1 and a kept reverse strand."""
    e = next(x for x in entries() if x[0] == "hand/local_finds_nothing/linear/0")
    assert [q for q in e[2]] == [b"CCCCCCCCCC", b"GGGGG", b"AAAA"]
    res = []
    for score, score_rev, rev, n, body in e[6]["plain"]:
        assert not isinstance(body, str)
        pairs = np.array(list(zip(A._undelta(body[0]), A._undelta(body[1]))), np.int32).reshape(n, 2)
        res.append(poa.QueryAlignment(score, score_rev, bool(rev), capi.VC_WIN_OK, pairs))
    other = [poa.QueryAlignment(7, 12, True, capi.VC_WIN_OK, np.array([[3, 0], [-1, 1], [5, -1], [6, 2]], np.int32)),
             poa.QueryAlignment(0, None, False, capi.VC_WIN_OVERFLOW, np.zeros((0, 2), np.int32)),
             poa.QueryAlignment(-9, None, False, capi.VC_WIN_OK, None)]
    text = poa.align_tsv(["c10", "g5", b"a4"], ["poly_a.fasta", "other.fa"], [res, other])
    assert text == (b"c10\tpoly_a.fasta\tOK\t0\t+\t*\n"
                    b"c10\tother.fa\tOK\t12\t-\t3:0,*:1,5:*,6:2\n"
                    b"g5\tpoly_a.fasta\tOK\t0\t+\t*\n"
                    b"g5\tother.fa\tOVERFLOW\t0\t+\t*\n"
                    b"a4\tpoly_a.fasta\tOK\t20\t+\t0:0,1:1,2:2,3:3\n"
                    b"a4\tother.fa\tOK\t-9\t+\t*\n")


# ------------------------------------------------------------------ the restatement against the reference
def test_fixture_shape():
    fx = load_align_fixture()
    assert len(fx["kat"]) == 18 and len(fx["groups"]) == 30 and len(fx["gaps"]) == 10
    assert {g["name"] for g in fx["hand"]} >= {"empty_query", "queries_for_an_empty_group", "byte_outside_the_graphs_alphabet",
                                               "local_finds_nothing", "query_of_length_1", "query_longer_than_every_path",
                                               "reverse_palindrome_tie"}
    es = entries()
    assert len(es) == 18 + 3 * (30 + 10 + len(fx["hand"]))
    for label, _, queries, squeries, _, _, e in es:
        assert len(e["plain"]) == len(e["strand"]) == len(queries) == len(squeries), label
        assert e["simd_agrees"] in (True, False)
    pal = next(x for x in es if x[0] == "hand/reverse_palindrome_tie/linear/1")[6]["strand"][0]
    assert pal[0] == pal[1] and pal[2] == 0 and pal[3] > 0                       # a tie stays as given
    assert any(r[2] for x in es for r in x[6]["strand"])
    assert all(r[3] == 0 and r[0] == 0 for r in next(x for x in es if x[0] == "hand/queries_for_an_empty_group/linear/1")[6]["plain"])


def _restate(a):
    mem, queries, squeries, t, scores = a
    eng, gr = A.build(mem, t, *scores)
    return [A.align_one(eng, gr, s, False) for s in queries], [A.align_one(eng, gr, s, True) for s in squeries]


def test_restatement_reproduces_every_fixture_entry():
    es = entries()
    with ProcessPoolExecutor(_workers()) as ex:
        got = list(ex.map(_restate, [(mem, q, sq, t, sc) for _, mem, q, sq, t, sc, _ in es], chunksize=2))
    n = 0
    for (label, *_, e), (plain, strand) in zip(es, got):
        for which, rs in (("plain", plain), ("strand", strand)):
            for k, (r, want) in enumerate(zip(rs, e[which])):
                assert A.same(r, want), (label, which, k, r["score"], r["score_rev"], want[:4])
                n += 1
    assert n == sum(len(x[6]["plain"]) + len(x[6]["strand"]) for x in es)
