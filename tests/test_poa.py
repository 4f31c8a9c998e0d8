"""CPU suite: the POA-group consensus (vc_poa_run, vechat_amd/poa.py) at its boundary -- declared and exported, arguments refused
before the device is touched, the batch marshalling, the command line's options -- and the fixture tests/golden/poa_groups.json.gz
pinned against the C oracle (local and global) and, where oracle/_ref was built, against the reference itself (all three types)."""
import ctypes as C
import gzip
import json
import os
import re

import numpy as np
import pytest

import oracle_api as oa
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _device_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:                                     # noqa: BLE001
        return os.path.exists("/dev/kfd")


def load_fixture():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_groups.json.gz"), "rt"))


def members(g):
    return [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]


def test_poa_entry_is_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    declared = set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert {"vc_poa_run", "vc_poa_last_error"} <= declared
    assert "typedef struct vc_poa_params" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run") and hasattr(lib, "vc_poa_last_error")
    assert C.sizeof(capi.VcPoaParams) == 20


def _call(lib, params, batch, null_spans=True, **override):
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    if null_spans:
        vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in override.items():
        setattr(vb, k, v)
    return lib.vc_poa_run(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r))


def _params(**kw):
    p = capi.VcPoaParams(device=0, algorithm=1, match=5, mismatch=-4, gap=-8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad = [
        ("null params", lambda: _call(lib, None, b)),
        ("algorithm -1", lambda: _call(lib, _params(algorithm=-1), b)),
        ("algorithm 3", lambda: _call(lib, _params(algorithm=3), b)),
        ("gap > 0", lambda: _call(lib, _params(gap=1), b)),
        ("match beyond int8", lambda: _call(lib, _params(match=128), b)),
        ("mismatch beyond int8", lambda: _call(lib, _params(mismatch=-129), b)),
        ("null win_seq_off", lambda: _call(lib, _params(), b, win_seq_off=None)),
        ("null seq_off", lambda: _call(lib, _params(), b, seq_off=None)),
        ("null bases", lambda: _call(lib, _params(), b, bases=None)),
        ("null quals beside a quality", lambda: _call(lib, _params(), b, quals=None)),
    ]
    wso = np.array([0, 3, 2], np.uint32)                  # a group that ends before it starts
    bad.append(("decreasing win_seq_off", lambda: _call(lib, _params(), b, win_seq_off=wso.ctypes.data_as(C.POINTER(C.c_uint32)))))
    wso1 = np.array([1, 2, 3], np.uint32)
    bad.append(("win_seq_off[0] != 0", lambda: _call(lib, _params(), b, win_seq_off=wso1.ctypes.data_as(C.POINTER(C.c_uint32)))))
    so = np.array([0, 4, 2, 6], np.uint64)
    bad.append(("decreasing seq_off", lambda: _call(lib, _params(), b, seq_off=so.ctypes.data_as(C.POINTER(C.c_uint64)))))
    long_b = poa.group_batch([["A" * 65535]])
    bad.append(("a sequence of 65 535 bases", lambda: _call(lib, _params(), long_b)))
    for what, f in bad:
        assert f() == capi.VC_ERR_ARG, what
        assert lib.vc_poa_last_error().decode(), what
    # a NULL quals is fine when no sequence has a quality; NULL spans and fasta flags always are
    fasta_only = poa.group_batch([["ACGT", "ACGA"], []])
    rc = _call(lib, _params(), fasta_only, quals=None)
    assert rc in (capi.VC_OK, capi.VC_ERR_NO_DEVICE)
    if not _device_visible():
        assert rc == capi.VC_ERR_NO_DEVICE


def test_valid_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    for alg in (0, 1, 2):
        for b in (poa.group_batch([["ACGT", ("ACGA", "IIII")], [], ["T"]]), poa.group_batch([])):
            assert _call(lib, _params(algorithm=alg, gap=0, match=127, mismatch=-128), b) == capi.VC_ERR_NO_DEVICE
            assert "device" in lib.vc_poa_last_error().decode()
    with pytest.raises(poa.PoaError) as e:
        poa.poa_consensus([["ACGT"]], "semi-global")
    assert e.value.rc == capi.VC_ERR_NO_DEVICE and "device" in str(e.value)


def test_group_batch_layout():
    b = poa.group_batch([["ACGT", ("GGA", "III"), b"T"], [], [("", ""), "", ("CA", b"#$")]])
    assert b.n_windows == 3
    assert b.win_seq_off.tolist() == [0, 3, 3, 6]
    assert b.seq_off.tolist() == [0, 4, 7, 8, 8, 8, 10]
    assert b.seq_has_qual.tolist() == [0, 1, 0, 1, 0, 1]
    assert b.bases[:10].tobytes() == b"ACGTGGATCA"
    assert b.quals[4:7].tobytes() == b"III" and b.quals[8:10].tobytes() == b"#$"
    assert not b.seq_begin.any() and not b.seq_end.any() and not b.win_fasta.any()
    assert poa.group_batch([]).n_windows == 0


def test_group_batch_rejections():
    with pytest.raises(ValueError, match="quality"):
        poa.group_batch([[("ACGT", "III")]])             # the reference throws: sequence and weights of unequal size
    with pytest.raises(ValueError):
        poa.group_batch([[("ACGT", "IIII", "x")]])
    with pytest.raises(TypeError):
        poa.group_batch(["ACGT"])                         # a group is a list of sequences
    with pytest.raises(TypeError):
        poa.group_batch([[123]])
    fx = load_fixture()
    bad = next(c for c in fx["invalid"] if "seqs" in c)
    with pytest.raises(ValueError):
        poa.group_batch([members(bad)])


def test_algorithm_names():
    assert [poa.algorithm_code(a) for a in ("local", "global", "semi-global", 0, 1, 2, np.int64(2))] == [0, 1, 2, 0, 1, 2, 2]
    for a in ("semiglobal", 3, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            poa.algorithm_code(a)


def test_command_line_options():
    a = poa.parse_args(["x.fa"])
    assert (a.m, a.n, a.g, a.l, a.device, a.files) == (5, -4, -8, 0, 0, ["x.fa"])
    a = poa.parse_args(["-m", "3", "-n", "-5", "-g", "-4", "-l", "2", "--device", "1", "a.fq", "b.fa.gz"])
    assert (a.m, a.n, a.g, a.l, a.device, a.files) == (3, -5, -4, 2, 1, ["a.fq", "b.fa.gz"])
    for argv in (["-e", "-2", "x.fa"], ["-q", "-24", "x.fa"], ["-c", "-1", "x.fa"], ["-l", "3", "x.fa"], ["-l", "-1", "x.fa"], []):
        with pytest.raises(SystemExit):
            poa.parse_args(argv)


def test_command_line_exits_1_on_bad_input(tmp_path, capsys):
    bad = tmp_path / "bad.fq"
    bad.write_text("@r\nACGT\n+\nIII\n")
    assert poa.main([str(bad)]) == 1
    assert "quality" in capsys.readouterr().err
    assert poa.main([str(tmp_path / "missing.fa")]) == 1


def test_fixture_shape():
    fx = load_fixture()
    assert set(fx["kat"]) == {"SemiGlobal", "SemiGlobalWithQualities"}
    sizes = {len(g["seqs"]) for g in fx["groups"]}
    assert {0, 1, 2, 3, 17, 64} <= sizes
    lens = [len(s) for g in fx["groups"] for s, _ in g["seqs"]]
    assert min(x for x in lens if x) == 1 and max(lens) > 1024
    assert any(q is None for g in fx["groups"] for _, q in g["seqs"]) and any(q is not None for g in fx["groups"] for _, q in g["seqs"])
    assert any("N" in s for g in fx["groups"] for s, _ in g["seqs"])
    assert len(fx["groups"]) >= 30 and all(set(g["expected"]) == {"0", "1", "2"} for g in fx["groups"])


def test_fixture_local_and_global_entries_match_the_oracle(built):
    lib = oa.load_oracle()
    fx = load_fixture()
    n = 0
    for g in fx["groups"]:
        mem = members(g)
        if not mem:
            continue
        for t in (0, 1):
            e = g["expected"][str(t)]
            got = oa.spoa_consensus(lib, "vco", [s for s, _ in mem], [q for _, q in mem], t, *g["scores"])
            assert e["status"] == capi.VC_WIN_OK and got.decode() == e["consensus"], (g["name"], t)
            n += 1
    assert n >= 56


@pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built (reference tree absent)")
def test_fixture_matches_the_reference(built):
    import sys
    sys.path.insert(0, GOLDEN)
    import make_poa
    fx = load_fixture()
    seqs, quals = __import__("fixtures").load_sample_reads()
    for name, k in fx["kat"].items():
        mem = list(zip(seqs, quals if k["quality"] else [None] * len(seqs)))
        assert make_poa.ref_consensus(oa.load_ref(), mem, 2, k["m"], k["n"], k["g"]) == (0, k["consensus"].encode()), name
    for kind in ("sse41", "sisd"):
        lib = oa.load_ref(kind)
        for g in fx["groups"]:
            for t in (0, 1, 2):
                e = g["expected"][str(t)]
                rc, c = make_poa.ref_consensus(lib, members(g), t, *g["scores"])
                assert (0 if rc == 0 else capi.VC_WIN_INVALID, c.decode()) == (e["status"], e["consensus"]), (kind, g["name"], t)
    # the bad inputs the reference accepts (an empty sequence, a group of empty ones, an empty group) are fixture groups, compared
    # with it above: VC_WIN_OK.  A quality string of the wrong length cannot be handed to vcref_spoa_consensus (it passes the
    # sequence's length as the quality's), so that case is pinned by graph.cpp:191-196 and test_group_batch_rejections.
    names = {g["name"]: g for g in fx["groups"]}
    for case in fx["invalid"]:
        if "group" in case:
            assert all(names[case["group"]]["expected"][str(t)]["status"] == capi.VC_WIN_OK for t in (0, 1, 2)), case
