"""CPU suite for the haplotype-aware correction of POA groups (vc_poa_run_correct, poa.poa_correct, the command line's
--correct): the entry at the library boundary, its argument checks before the device, Python's own validation, the command line's
refusals, the FASTA writer, the fixture's shape, and the CPU restatement tests/poa_correct_ref.py against every entry of
tests/golden/poa_correct.json.gz (recorded from the reference by tests/golden/make_poa_correct.py)."""
import ctypes as C
import gzip
import json
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import poa_correct_ref as PC
from poa_common import _gp, _workers
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _device_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return os.path.exists("/dev/kfd")


def load_correct_fixture():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_correct.json.gz"), "rt"))


def entries():
    """-> [(label, members [(bytes, bytes | None)], entry)] of every fixture entry"""
    by_name = {g["name"]: g["seqs"] for g in json.load(gzip.open(os.path.join(GOLDEN, "poa_groups.json.gz"), "rt"))["groups"]}
    out = []
    for e in load_correct_fixture()["entries"]:
        seqs = e["seqs"] if "seqs" in e else by_name[e["group"]]
        mem = [(s.encode("latin-1"), None if q is None else q.encode("latin-1")) for s, q in seqs]
        out.append((f"{e['kind']}:{e.get('name') or e['group']}:{e['type']}:{e.get('model', '')}:{e['num_prune']}", mem, e))
    return out


# ------------------------------------------------------------------ the boundary
def test_correct_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_correct" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_correct")
    for name, cls in (("vc_poa_correct_out", capi.VcPoaCorrectOut), ("vc_poa_prune_params", capi.VcPoaPruneParams)):
        body = hdr[hdr.index(f"typedef struct {name}"):hdr.index(f"}} {name};")]
        fields = [f for decl in re.findall(r"([^;{]+);", body) for f in re.findall(r"(\w+)\s*(?:,|$)", decl.split("*")[-1].strip())]
        assert fields == [f for f, _ in cls._fields_], (name, fields)
    assert C.sizeof(capi.VcPoaCorrectOut) == 48 and capi.VcPoaCorrectOut.bytes.offset == 40
    assert C.sizeof(capi.VcPoaPruneParams) == 24 and capi.VcPoaPruneParams.num_prune.offset == 16
    assert capi.load_hip().vc_poa_run_correct.argtypes == [C.POINTER(capi.VcBatch), C.POINTER(capi.VcPoaGapParams),
                                                           C.POINTER(capi.VcPoaPruneParams), C.POINTER(capi.VcResult),
                                                           C.POINTER(capi.VcPoaCorrectOut)]
    assert C.sizeof(capi.VcPoaAlignOut) == 80 and C.sizeof(capi.VcPoaGraphOut) == 152 and C.sizeof(capi.VcPoaMsaOut) == 72   # unchanged


def _call(lib, params, batch, prune=(0.22, 0.19, 3), out=True, boverride=None):
    """-> (rc, the library's message, the correction output)"""
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in (boverride or {}).items():
        setattr(vb, k, v)
    co = capi.VcPoaCorrectOut()
    co.status = C.cast(1, C.POINTER(C.c_uint8))                                 # a failed call must leave every pointer NULL
    pr = capi.VcPoaPruneParams(*prune) if prune is not None else None
    rc = lib.vc_poa_run_correct(C.byref(vb), C.byref(params) if params is not None else None, C.byref(pr) if pr is not None else None,
                                C.byref(r), C.byref(co) if out else None)
    return rc, lib.vc_poa_last_error().decode(), co


def test_correct_argument_errors_come_before_the_device_in_the_documented_order(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    dec = (C.c_uint64 * 4)(0, 3, 2, 5)
    nan = float("nan")
    # one defect each, in the documented order: 1 as vc_poa_run_gaps (the batch included), 2 num_prune, 3 the thresholds
    bad = [("null params", lambda: _call(lib, None, b), "null argument"),
           ("null prune params", lambda: _call(lib, _gp(), b, prune=None), "null argument"),
           ("null output", lambda: _call(lib, _gp(), b, out=False), "null argument"),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b), "algorithm"),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b), "opening"),
           ("gap_extend2 > 0", lambda: _call(lib, _gp(gap_extend2=1), b), "extension"),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b), "-128..127"),
           ("batch offsets decrease", lambda: _call(lib, _gp(), b, boverride=dict(seq_off=dec)), "seq_off decreases"),
           ("num_prune 0", lambda: _call(lib, _gp(), b, (0.22, 0.19, 0)), "num_prune"),
           ("confidence NaN", lambda: _call(lib, _gp(), b, (nan, 0.19, 3)), "min_confidence"),
           ("confidence negative", lambda: _call(lib, _gp(), b, (-0.1, 0.19, 3)), "min_confidence"),
           ("support NaN", lambda: _call(lib, _gp(), b, (0.22, nan, 3)), "min_support"),
           ("support negative", lambda: _call(lib, _gp(), b, (0.22, -1e-9, 3)), "min_support")]
    for what, f, msg in bad:
        rc, text, co = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (what, rc, text)
        assert what == "null output" or (not co.status and not co.score and not co.corr_off and not co.corr), what
    # two defects: the earlier check answers
    order = [(lambda: _call(lib, _gp(algorithm=3), b, (nan, nan, 0)), "algorithm"),
             (lambda: _call(lib, _gp(match=128), b, (0.22, 0.19, 0)), "-128..127"),
             (lambda: _call(lib, _gp(), b, (nan, 0.19, 0), boverride=dict(seq_off=dec)), "seq_off decreases"),
             (lambda: _call(lib, _gp(), b, (nan, -1.0, 0)), "num_prune"),
             (lambda: _call(lib, _gp(), b, (-1.0, nan, 1)), "min_confidence")]
    for f, msg in order:
        rc, text, _ = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (msg, rc, text)
    if not _device_visible():                                                   # valid arguments reach the device check, and only then
        for prune in ((0.22, 0.19, 3), (0.0, 0.0, 1), (float("inf"), 5.0, 7)):
            rc, text, co = _call(lib, _gp(), b, prune)
            assert rc == capi.VC_ERR_NO_DEVICE and not co.status, (prune, rc, text)


def test_poa_correct_validates_its_arguments_before_any_call():
    g = [["ACGT", "ACGA"]]
    for kw, msg in ((dict(prune_rounds=0), "prune_rounds"), (dict(prune_rounds=-1), "prune_rounds"), (dict(prune_rounds=2.0), "prune_rounds"),
                    (dict(prune_rounds=True), "prune_rounds"), (dict(min_confidence=float("nan")), "min_confidence"),
                    (dict(min_confidence=-0.5), "min_confidence"), (dict(min_support=-1), "min_support"),
                    (dict(min_support="0.2"), "min_support"), (dict(algorithm="banded"), "algorithm")):
        with pytest.raises(ValueError, match=msg):
            poa.poa_correct(g, **kw)
    with pytest.raises(ValueError, match="quality string"):
        poa.poa_correct([[("ACGT", "II")]])
    with pytest.raises(TypeError):
        poa.poa_correct(["ACGT"])


def test_command_line_refuses_what_does_not_go_with_correct(capsys, tmp_path):
    f = os.path.join(GOLDEN, "sample.fastq.gz")
    out = str(tmp_path / "c.fa")
    for extra in (["-r", "1"], ["-r", "2"], ["--gfa"], ["--gfa-consensus"], ["--graphviz", str(tmp_path / "g.dot")], ["--both-strands"],
                  ["--align", f, "--align-out", str(tmp_path / "a.tsv")]):
        assert poa.main(["--correct", out, *extra, f]) == 1, extra
        assert "--correct does not go with" in capsys.readouterr().err, extra
        assert not os.path.exists(out)
    a = poa.parse_args(["--correct", out, f])
    assert (a.min_confidence, a.min_support, a.prune_rounds) == (0.22, 0.19, 3)
    a = poa.parse_args(["--correct", out, "--min-confidence", "0.3", "--min-support", "0.1", "--prune-rounds", "2", f])
    assert (a.min_confidence, a.min_support, a.prune_rounds) == (0.3, 0.1, 2)


def test_fasta_writer_on_a_fixture_entry():
    label, mem, e = next(x for x in entries() if x[2].get("name") == "unrelated_member" and x[2]["type"] == 0)
    reads = [s.encode("latin-1") for s in e["expected"]["reads"]]
    assert b"" in reads and any(reads)
    records = [[(f"read/{i}", s, q) for i, (s, q) in enumerate(mem)], [(b"solo", b"ACGT", None)]]
    res = [poa.Corrected(e["expected"]["consensus"].encode(), reads, None, None), poa.Corrected(b"ACGT", [b"ACGT"], None, None)]
    text = poa.corrected_fasta(records, res)
    want = b"".join(b">read/%d\n%s\n" % (i, r) for i, r in enumerate(reads)) + b">solo\nACGT\n"
    assert text == want and b"\n\n" in text                                    # an empty correction keeps its record, with an empty line


def test_fixture_shape():
    fx = load_correct_fixture()
    es = fx["entries"]
    assert fx["params"]["generator"] == "tests/golden/make_poa_correct.py"
    kinds = {k: [e for e in es if e["kind"] == k] for k in ("groups", "gaps", "hap", "hand")}
    assert len(kinds["groups"]) == 60 and {e["type"] for e in kinds["groups"]} == {0, 1}
    assert len(kinds["gaps"]) == 20 and {e["model"] for e in kinds["gaps"]} == {"affine", "convex"}
    assert {e["num_prune"] for e in kinds["hap"]} == {1, 2, 3} and len(kinds["hap"]) == 18
    assert {e["name"] for e in kinds["hand"]} == {"empty_member_first", "empty_members_only", "unrelated_member", "one_member", "length_1",
                                                  "two_components"}
    assert all(e["simd_agrees"] for e in es)
    for e in es:
        x = e["expected"]
        assert len(x["scores"]) == len(x["lens"]) and (isinstance(x["reads"], str) or [len(r) for r in x["reads"]] == x["lens"])
    # what the generator asserted, from the recorded data
    assert any(e["stats"]["pruned"] for e in es) and any(e["stats"]["lost"] for e in es) and all(e["stats"]["created"] == 0 for e in es)
    assert any(0 in e["expected"]["lens"] and e.get("name") == "unrelated_member" for e in es)
    assert any(isinstance(e["expected"]["reads"], str) for e in es) and sum(not isinstance(e["expected"]["reads"], str) for e in es) > 60
    biggest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "poa_correct.json.gz")
    assert os.path.getsize(os.path.join(GOLDEN, "poa_correct.json.gz")) <= biggest


def _restate(a):
    mem, e = a
    r = PC.correct_group(mem, e["type"], *e["scores"], e["min_confidence"], e["min_support"], e["num_prune"])
    return PC.same(r, e["expected"]), r["stats"]


def test_restatement_reproduces_every_fixture_entry():
    es = entries()
    with ProcessPoolExecutor(_workers()) as ex:
        got = list(ex.map(_restate, [(mem, e) for _, mem, e in es], chunksize=2))
    for (label, _, e), (diff, stats) in zip(es, got):
        assert diff == "" and stats == e["stats"], (label, diff, stats, e["stats"])
