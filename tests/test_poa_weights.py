"""CPU suite: explicit weights and the consensus profile of POA groups (vc_poa_run_weighted, the weights= keyword and poa_profile of
vechat_amd.poa, --weights / --profile): the restatement tests/poa_weights_ref.py reproduces every entry of the reference's fixture, the nine runs on the 55 reads a case each;
the Python layer's validation; the command line's parsing and refusals; the entry's argument checks, which return before the
device is touched.  The symbol does not exist before this entry was added, so the argument tests fail without it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import poa_weights_cases as cases
import poa_weights_ref as W
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.cases()


def test_fixture_has_every_section():
    fx = cases.load()
    assert len(fx["kat"]) == 9 and len(fx["groups"]) == 30 and len(fx["gaps"]) == 10 and len(fx["strand"]) == 10
    names = {h["name"] for h in fx["hand"]}
    assert {"heavy_minority", "zero_weight_member", "uint32_wrap", "starts_inside_ends_early", "insertion", "deletion",
            "three_codes_in_a_column", "code_only_off_consensus", "local_finds_nothing", "empty_members", "empty_group", "group_of_one",
            "consensus_length_63", "consensus_length_64", "consensus_length_65", "consensus_length_129", "seventy_members"} <= names


def _reproduces(case):
    cid, members, weights, t, sc, strands, e = case
    r = W.run(members, weights, t, *sc, strands=strands)
    cases.check(r, e, cid)
    nc = len(r["codes"])
    sums = [sum(r["counts"][k][j] for k in range(nc)) for j in range(len(r["consensus"]))]
    assert (sums == r["coverage"]) == e["rows_sum_to_coverage"], cid
    assert r["coverage"] == e["coverage"], cid


SMALL = [c for c in CASES if not c[0].startswith("kat")]


@pytest.mark.parametrize("chunk", range(8))
def test_restatement_reproduces_the_fixture(chunk):
    for case in SMALL[chunk::8]:
        _reproduces(case)


@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("kat")], ids=lambda c: c[0])
def test_restatement_reproduces_the_known_answer_runs(case):
    """the 55 sample reads, three algorithms x per-read weights, per-base weights, no weights: a case each"""
    _reproduces(case)


def test_python_validation():
    g = [[b"ACGT", b"ACG"]]
    for bad in ([[None]], [[None, -1]], [[None, 1 << 32]], [[None, [1, 2]]], [[None, "12"]], [[None, [1, 2, 1 << 32]]], [[None, 1.5]],
                [[None, [1, 2, True]]], [None, None]):
        with pytest.raises(ValueError, match="group 0|weight lists"):
            poa.weight_arrays(g, bad)
    assert poa.weight_arrays(g, None) is None and poa.weight_arrays(g, [None]) is None and poa.weight_arrays(g, [[None, None]]) is None
    mode, sw, bw = poa.weight_arrays(g, [[7, [1, 2, 3]]])
    assert mode.tolist() == [1, 2] and sw.tolist() == [7, 0] and bw.tolist() == [0, 0, 0, 0, 1, 2, 3]
    for f in (lambda: poa.poa_extend([], [], weights=[]), lambda: poa.poa_align([[b"A"]], [[b"A"]], weights=[[1]]),
              lambda: poa.poa_correct([[b"A"]], weights=[[1]]), lambda: poa.poa_graph([[b"A"]], resumable=True, weights=[[1]])):
        with pytest.raises(ValueError, match="takes neither weights nor the profile"):
            f()
    with pytest.raises(ValueError, match="do not go with"):
        poa._run(poa.group_batch(g), None, spans=(np.zeros(2, np.uint32),) * 2, profile=True)


def test_weight_file_parsing(tmp_path):
    recs = [[(b"r1", b"ACGT", None), (b"r2", b"AC", None)], [(b"r1", b"GG", None)]]
    files = ["a.fa", "b.fa"]
    got = poa.parse_weights(b"# c\na.fa\tr2\t3,4\n\nb.fa\tr1\t37\n", files, recs)
    assert got == [[None, [3, 4]], [37]]
    for bad, msg in ((b"a.fa\tr2\n", "expected"), (b"a.fa\tr2\t-1\n", "expected"), (b"c.fa\tr2\t1\n", "no input file"),
                     (b"a.fa\tr9\t1\n", "has no record"), (b"a.fa\tr2\t1\na.fa\tr2\t2\n", "listed twice"), (b"a.fa\tr2\t1,2,3\n", "3 weights for the 2 bases"),
                     (b"a.fa\tr2\t4294967296\n", "not in 0")):
        with pytest.raises(ValueError, match=msg):
            poa.parse_weights(bad, files, recs)
    pr = poa.Profile(b"AC", b"AC", np.array([[2, 0], [0, 1], [0, 1]], np.uint32), 0)
    assert poa.profile_tsv(["g"], [pr]) == b"#group\tpos\tbase\tA\tC\tgaps\ng\t0\tA\t2\t0\t0\ng\t1\tC\t0\t1\t1\n"


@pytest.mark.parametrize("other", (["--align", "q.fa", "--align-out", "o"], ["--correct", "c.fa"], ["--spans", "s.tsv"], ["--save-graphs", "g.npz"],
                                   ["--from-graphs", "g.npz"]))
@pytest.mark.parametrize("opt", ("--weights", "--profile"))
def test_command_line_refusals(opt, other, capsys):
    assert poa.main([opt, "x.tsv", *other, "a.fa"]) == 1
    assert "--weights / --profile do not go with" in capsys.readouterr().err


def test_header_library_and_binding(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_weighted" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_weight_in" in hdr and "typedef struct vc_poa_profile_out" in hdr
    assert "the verbose per-code summary is not offered" not in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert len(capi.load_hip().vc_poa_run_weighted.argtypes) == 8


def _call(mode, seq_w, base_w, prof=True, wnull=False, p=None):
    lib = capi.load_hip()
    batch = poa.group_batch([[b"ACGT", b"ACG"], [b"AC", b"AC", b"A"]])
    cons, off, status, r, vb = poa._result_buffers(batch)
    keep = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in ((mode, np.uint8), (seq_w, np.uint32), (base_w, np.uint32))]
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))     # noqa: E731
    w = capi.VcPoaWeightIn(ptr(keep[0], C.c_uint8), ptr(keep[1], C.c_uint32), ptr(keep[2], C.c_uint32))
    po = capi.VcPoaProfileOut(n_groups=99)
    p = p or capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    rc = lib.vc_poa_run_weighted(C.byref(p), None if wnull else C.byref(w), C.byref(vb), C.byref(r), None, None, None, C.byref(po) if prof else None)
    return rc, lib.vc_poa_last_error().decode(), po


def test_argument_checks_in_order(built):
    """every VC_ERR_ARG of the entry, in the header's order, each with the later violations present too"""
    bad_p = capi.VcPoaGapParams(device=0, algorithm=7, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    rc, msg, po = _call(None, None, None, p=bad_p)
    assert rc == capi.VC_ERR_ARG and "algorithm" in msg and not po.counts and not po.n_codes
    rc, msg, _ = _call(None, None, None)
    assert rc == capi.VC_ERR_ARG and "null weight mode" in msg
    # a mode above 2 comes before a NULL seq_weight or base_weight, wherever the members stand
    rc, msg, _ = _call([2, 0, 1, 3, 2], None, None)
    assert rc == capi.VC_ERR_ARG and "member 1 of group 1" in msg and "not 0, 1 or 2" in msg
    # then seq_weight beside a mode-1 member, before base_weight beside an earlier mode-2 member
    rc, msg, _ = _call([0, 2, 0, 1, 1], None, None)
    assert rc == capi.VC_ERR_ARG and "member 1 of group 1" in msg and "seq_weight" in msg
    rc, msg, _ = _call([0, 1, 0, 0, 2], [0] * 5, None)
    assert rc == capi.VC_ERR_ARG and "member 2 of group 1" in msg and "base_weight" in msg
    rc, msg, _ = _call([0, 2, 0, 0, 2], None, None)
    assert rc == capi.VC_ERR_ARG and "member 1 of group 0" in msg and "base_weight" in msg


def test_null_mode_is_refused_whatever_the_batch_holds(built):
    lib = capi.load_hip()
    batch = poa.group_batch([])
    cons, off, status, r, vb = poa._result_buffers(batch)
    p = capi.VcPoaGapParams(device=0, algorithm=1, match=5, mismatch=-4, gap_open=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8)
    rc = lib.vc_poa_run_weighted(C.byref(p), C.byref(capi.VcPoaWeightIn()), C.byref(vb), C.byref(r), None, None, None, None)
    assert rc == capi.VC_ERR_ARG and "null weight mode" in lib.vc_poa_last_error().decode()


def test_no_device_only_after_the_checks(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a device")
    rc, msg, po = _call([0, 1, 2, 0, 0], [1] * 5, [1] * 10)
    assert rc == capi.VC_ERR_NO_DEVICE and not po.counts
    rc, _, _ = _call(None, None, None, wnull=True)
    assert rc == capi.VC_ERR_NO_DEVICE
