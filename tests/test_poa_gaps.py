"""CPU suite: affine and convex gaps for the POA-group consensus (vc_poa_run_gaps, poa_consensus(..., gap_extend=...), the
command line's --gap-extend / --gap-open2 / --gap-extend2) at their boundary -- declared and exported, spoa's subtype rule, the
arguments refused before the device -- and the CPU restatement tests/poa_gaps_ref.py, which is the bar for the device: one row's
two-pass scans against spoa's column loop, spoa's 18 known answers, every linear entry of poa_groups.json.gz, and entries of
poa_gaps_groups.json.gz recomputed."""
import ctypes as C
import gzip
import json
import os
import random
import re
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import fixtures
import poa_gaps_ref as R
from poa_common import TYPES, _gp, _workers
from test_poa import _device_visible, load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_kats():
    return json.load(open(os.path.join(GOLDEN, "spoa_kat_gaps.json")))


def load_gaps_fixture():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_gaps_groups.json.gz"), "rt"))


def test_gap_entry_is_declared_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_gaps" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "typedef struct vc_poa_gap_params" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_gaps")
    assert C.sizeof(capi.VcPoaGapParams) == 32
    assert [f for f, _ in capi.VcPoaGapParams._fields_] == ["device", "algorithm", "match", "mismatch", "gap_open", "gap_extend",
                                                             "gap_open2", "gap_extend2"]
    assert C.sizeof(capi.VcPoaParams) == 20                     # vc_poa_params is unchanged


# ------------------------------------------------------------------ spoa's subtype rule (alignment_engine.cpp:59-69)
RULE = [
    # (g, e, q, c) -> (subtype, g, e, q, c)
    ((-8, -8, -8, -8), ("linear", -8, -8, -8, -8)),
    ((-4, -6, -10, -2), ("linear", -4, -4, -10, -2)),            # g > e: linear, e = g; q and c kept as given
    ((-6, -6, -10, -2), ("linear", -6, -6, -10, -2)),            # g == e: linear
    ((-8, -6, -8, -6), ("affine", -8, -6, -8, -6)),
    ((-8, -6, -8, -2), ("affine", -8, -6, -8, -6)),              # g == q: affine, q = g and c = e
    ((-8, -6, -4, -2), ("affine", -8, -6, -8, -6)),              # g < q: affine
    ((-8, -6, -10, -6), ("affine", -8, -6, -8, -6)),             # e == c: affine
    ((-8, -2, -10, -6), ("affine", -8, -2, -8, -2)),             # e > c: affine
    ((-8, -6, -10, -2), ("convex", -8, -6, -10, -2)),            # spoa's convex known-answer tests
    ((-8, -6, -10, -4), ("convex", -8, -6, -10, -4)),            # spoa's command-line defaults
    ((-1, 0, -2, 0), ("affine", -1, 0, -1, 0)),
    ((-2, -1, -3, 0), ("convex", -2, -1, -3, 0)),
]


def test_gap_model_rule():
    for args, want in RULE:
        assert poa.gap_model(*args) == want, args
        assert R.gap_model(*args) == (R.SUBTYPES[want[0]],) + want[1:], args
    # spoa's shorter overloads: Create(g) = (g, g, g, g), Create(g, e) = (g, e, g, e)
    assert poa.gap_model(-8) == ("linear", -8, -8, -8, -8)
    assert poa.gap_model(-8, -6) == ("affine", -8, -6, -8, -6)
    assert poa.gap_model(-8, -6, -10) == ("affine", -8, -6, -8, -6)   # c = e: affine
    assert poa.gap_model(-8, -6, -10, -2) == ("convex", -8, -6, -10, -2)


# ------------------------------------------------------------------ the C ABI's checks
def _call(lib, params, batch, **override):
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in override.items():
        setattr(vb, k, v)
    return lib.vc_poa_run_gaps(C.byref(params) if params is not None else None, C.byref(vb), C.byref(r))


def test_gap_argument_errors_come_before_the_device(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad = [("null params", lambda: _call(lib, None, b)),
           ("algorithm -1", lambda: _call(lib, _gp(algorithm=-1), b)),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b)),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b)),
           ("gap_open2 > 0", lambda: _call(lib, _gp(gap_open2=1), b)),
           ("gap_extend > 0", lambda: _call(lib, _gp(gap_extend=1), b)),
           ("gap_extend2 > 0", lambda: _call(lib, _gp(gap_extend2=2), b)),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b)),
           ("mismatch beyond int8", lambda: _call(lib, _gp(mismatch=-129), b)),
           ("gap_open beyond int8", lambda: _call(lib, _gp(gap_open=-129), b)),
           ("gap_extend beyond int8", lambda: _call(lib, _gp(gap_extend=-129), b)),
           ("gap_open2 beyond int8", lambda: _call(lib, _gp(gap_open2=-200), b)),
           ("gap_extend2 beyond int8", lambda: _call(lib, _gp(gap_extend2=-129), b)),
           ("null win_seq_off", lambda: _call(lib, _gp(), b, win_seq_off=None)),
           ("null seq_off", lambda: _call(lib, _gp(), b, seq_off=None)),
           ("null bases", lambda: _call(lib, _gp(), b, bases=None)),
           ("null quals beside a quality", lambda: _call(lib, _gp(), b, quals=None))]
    long_b = poa.group_batch([["A" * 65535]])
    bad.append(("a sequence of 65 535 bases", lambda: _call(lib, _gp(), long_b)))
    for what, f in bad:
        assert f() == capi.VC_ERR_ARG, what
        assert lib.vc_poa_last_error().decode(), what
    # spoa's order: the opening penalties are checked before the extensions, both before the int8 range
    assert _call(lib, _gp(gap_open=1, gap_extend=1), b) == capi.VC_ERR_ARG
    assert "opening" in lib.vc_poa_last_error().decode()
    assert _call(lib, _gp(gap_extend=1, match=500), b) == capi.VC_ERR_ARG
    assert "extension" in lib.vc_poa_last_error().decode()


def test_valid_gap_arguments_without_a_device(built):
    if _device_visible():
        pytest.skip("a HIP device is visible")
    lib = capi.load_hip()
    for alg in (0, 1, 2):
        for g, e, q, c in ((-8, -8, -8, -8), (-8, -6, -8, -6), (-8, -6, -10, -2), (0, 0, 0, 0), (-128, -128, -128, -128)):
            for b in (poa.group_batch([["ACGT", ("ACGA", "IIII")], [], ["T"]]), poa.group_batch([])):
                p = _gp(algorithm=alg, gap_open=g, gap_extend=e, gap_open2=q, gap_extend2=c, match=127, mismatch=-128)
                assert _call(lib, p, b) == capi.VC_ERR_NO_DEVICE
                assert "device" in lib.vc_poa_last_error().decode()
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_consensus([["ACGT"]], "semi-global", gap_extend=-6)
    assert ex.value.rc == capi.VC_ERR_NO_DEVICE and "vc_poa_run_gaps" in str(ex.value)


# ------------------------------------------------------------------ poa_consensus's keywords
class _Recorder:
    """stands in for the library: records which entry was called with which scores, returns every group empty and OK"""

    def __init__(self):
        self.calls = []

    def _rec(self, name, p):
        self.calls.append((name, {f: getattr(p._obj, f) for f, _ in p._obj._fields_}))
        return 0

    def vc_poa_run(self, p, b, r):
        return self._rec("vc_poa_run", p)

    def vc_poa_run_gaps(self, p, b, r):
        return self._rec("vc_poa_run_gaps", p)

    def vc_poa_last_error(self):
        return b""


def test_poa_consensus_gap_keywords():
    lib = _Recorder()
    g = [["ACGT", "ACGA"]]
    poa.poa_consensus(g, "global", 5, -4, -8, lib=lib)
    poa.poa_consensus(g, "local", 3, -5, -4, 0, True, lib)               # every existing positional call is unchanged
    poa.poa_consensus(g, "global", gap=-8, gap_extend=-6, lib=lib)
    poa.poa_consensus(g, "global", gap=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4, lib=lib)
    poa.poa_consensus(g, 2, gap=-8, gap_open2=-10, lib=lib)
    poa.poa_consensus(g, 2, gap=-8, gap_extend2=-2, lib=lib)
    poa.poa_consensus(g, 2, gap=-8, gap_extend=-8, gap_open2=-8, gap_extend2=-8, lib=lib)
    names = [n for n, _ in lib.calls]
    assert names == ["vc_poa_run"] * 2 + ["vc_poa_run_gaps"] * 5
    assert lib.calls[0][1] == dict(device=0, algorithm=1, match=5, mismatch=-4, gap=-8)
    assert lib.calls[1][1] == dict(device=0, algorithm=0, match=3, mismatch=-5, gap=-4)
    gaps = [tuple(p[k] for k in ("gap_open", "gap_extend", "gap_open2", "gap_extend2")) for _, p in lib.calls[2:]]
    assert gaps == [(-8, -6, -8, -6), (-8, -6, -10, -4), (-8, -8, -10, -8), (-8, -8, -8, -2), (-8, -8, -8, -8)]
    assert lib.calls[3][1]["algorithm"] == 1 and lib.calls[4][1]["algorithm"] == 2
    with pytest.raises(TypeError):
        poa.poa_consensus(g, "global", 5, -4, -8, 0, True, lib, -6)   # keyword-only
    assert poa.poa_consensus([["ACGT"], []], gap_extend=-6, lib=_Recorder()) == [b"", b""]


# ------------------------------------------------------------------ the command line
def test_command_line_gap_options(monkeypatch, tmp_path):
    a = poa.parse_args(["x.fa"])
    assert (a.g, a.gap_extend, a.gap_open2, a.gap_extend2) == (-8, None, None, None)
    a = poa.parse_args(["-l", "1", "--gap-extend", "-6", "--gap-open2", "-10", "--gap-extend2", "-4", "x.fa"])
    assert (a.l, a.g, a.gap_extend, a.gap_open2, a.gap_extend2, a.files) == (1, -8, -6, -10, -4, ["x.fa"])
    a = poa.parse_args(["--gap-extend=-6", "x.fa"])
    assert a.gap_extend == -6
    # spoa's short options stay refused: argparse must not take them for the long ones (prefix matching)
    for argv in (["-e", "-6", "x.fa"], ["-q", "-10", "x.fa"], ["-c", "-4", "x.fa"], ["-e-6", "x.fa"], ["--gap-e", "-6", "x.fa"]):
        with pytest.raises(SystemExit):
            poa.parse_args(argv)
    got = []
    monkeypatch.setattr(poa, "poa_consensus", lambda groups, *args, **kw: got.append((args, kw)) or [b"AC"] * len(groups))
    fa = tmp_path / "x.fa"
    fa.write_text(">r\nACGT\n")
    assert poa.main(["-l", "2", "--gap-extend", "-6", "--gap-open2", "-10", str(fa)]) == 0
    assert got[0][0] == (2, 5, -4, -8)
    assert {k: got[0][1][k] for k in ("gap_extend", "gap_open2", "gap_extend2")} == dict(gap_extend=-6, gap_open2=-10, gap_extend2=None)
    assert poa.main([str(fa)]) == 0
    assert {k: got[1][1][k] for k in ("gap_extend", "gap_open2", "gap_extend2")} == dict(gap_extend=None, gap_open2=None, gap_extend2=None)
    assert "-g-8--gap-extend-6--gap-open2-10--gap-extend2-4" in "".join(_help().split())     # (argparse wraps at hyphens)
    assert "linear" in poa.__doc__ and "convex" in poa.__doc__


def _help():
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        poa.parse_args(["--help"])
    return buf.getvalue()


# ------------------------------------------------------------------ the restatement: one row
def test_row_scans_equal_spoas_column_loop():
    """The two-pass model of a row (tests/poa_gaps_ref.row_scan, what k_lg_fwd computes) against spoa's sequential recurrence,
    on random rows of all three subtypes, kSW's clamp included."""
    rng = random.Random(20261016)
    n_rows = 0
    for sub in (R.LINEAR, R.AFFINE, R.CONVEX):
        for _ in range(1500):
            while True:
                g, e, q, c = (rng.randint(-20, 0) for _ in range(4))
                s, g, e, q, c = R.gap_model(g, e, q, c)
                if s == sub:
                    break
            sw = rng.random() < 0.3
            n = rng.randint(1, 70)
            h0 = 0 if sw or rng.random() < 0.3 else rng.randint(-400, 0)
            base = rng.randint(-300, 50)
            d = [base + rng.randint(-40, 40) for _ in range(n)]
            f = [base + rng.randint(-60, 20) for _ in range(n)]
            o = [base + rng.randint(-60, 20) for _ in range(n)]
            H, E, Q = R.row_sequential(sub, sw, d, f, o, h0, g, e, q, c)
            x = np.maximum(np.array(d), np.array(f) if sub != R.LINEAR else np.array(f))
            if sub == R.CONVEX:
                x = np.maximum(x, np.array(o))
            if sw:
                x = np.maximum(x, 0)
            h2, e2, q2 = R.row_scan(sub, x, h0, g, e, q, c)
            assert h2.tolist() == H, (sub, sw, g, e, q, c)
            assert (e2 is None and E is None) or e2.tolist() == E, (sub, sw, g, e, q, c)
            assert (q2 is None and Q is None) or q2.tolist() == Q, (sub, sw, g, e, q, c)
            n_rows += 1
    # E and Q taken from scans over x instead of the final H are not spoa's for convex rows (why the device scans twice)
    differ = 0
    for _ in range(500):
        g, e, q, c = -8, -6, -10, -2
        n = 40
        d = [rng.randint(-60, 30) for _ in range(n)]
        f = [rng.randint(-80, 0) for _ in range(n)]
        o = [rng.randint(-80, 0) for _ in range(n)]
        H, E, Q = R.row_sequential(R.CONVEX, False, d, f, o, -20, g, e, q, c)
        x = np.maximum(np.maximum(np.array(d), np.array(f)), np.array(o))
        differ += R._excl(-20, x, e, g).tolist() != E or R._excl(-20, x, c, q).tolist() != Q
    assert differ > 0
    assert n_rows == 4500


# ------------------------------------------------------------------ the restatement: spoa's known answers and the linear fixture
def _kat_job(name):
    k = load_kats()[name]
    seqs, quals = fixtures.load_sample_reads()
    mem = [(s, q if k["quality"] else None) for s, q in zip(seqs, quals)]
    return name, R.consensus(mem, TYPES[k["type"]], k["m"], k["n"], k["g"], k["e"], k["q"], k["c"]).decode()


def test_restatement_reproduces_spoas_known_answers():
    kats = load_kats()
    assert len(kats) == 18
    subtypes = [R.gap_model(k["g"], k["e"], k["q"], k["c"])[0] for k in kats.values()]
    assert subtypes.count(R.LINEAR) == 6 and subtypes.count(R.AFFINE) == 6 and subtypes.count(R.CONVEX) == 6
    linear = fixtures.load_kats()                                  # the four of spoa_kat.json are the same strings
    assert all(kats[n]["consensus"] == k["consensus"] for n, k in linear.items())
    with ProcessPoolExecutor(_workers()) as ex:
        got = dict(ex.map(_kat_job, sorted(kats, key=lambda n: "Convex" not in n)))
    for name, k in kats.items():
        assert got[name] == k["consensus"], name


def _fixture_job(a):
    gi, t = a
    g = load_fixture()["groups"][gi]
    try:
        return gi, t, 0, R.consensus(members(g), t, *g["scores"]).decode()
    except ValueError:
        return gi, t, capi.VC_WIN_INVALID, ""


def test_restatement_reproduces_the_linear_fixture():
    groups = load_fixture()["groups"]
    jobs = sorted(((gi, t) for gi in range(len(groups)) for t in (0, 1, 2)),
                  key=lambda a: -len(groups[a[0]]["seqs"]) * sum(len(s) for s, _ in groups[a[0]]["seqs"]))
    with ProcessPoolExecutor(_workers()) as ex:
        for gi, t, st, c in ex.map(_fixture_job, jobs):
            e = groups[gi]["expected"][str(t)]
            assert (st, c) == (e["status"], e["consensus"]), (groups[gi]["name"], t)
    assert len(jobs) == 90


def _gaps_job(a):
    name, key, t = a
    sys.path.insert(0, GOLDEN)
    import make_poa_gaps
    g = next(g for g in load_fixture()["groups"] if g["name"] == name)
    return a, make_poa_gaps.expected(g, t, make_poa_gaps.SCORES[key])


def test_gaps_fixture_shape_and_entries():
    fx = load_gaps_fixture()
    names = [g["name"] for g in load_fixture()["groups"]]
    assert sorted(fx["groups"]) == sorted(names)
    kinds = {key: poa.gap_model(*s[2:])[0] for key, s in fx["scores"].items()}
    assert sorted(kinds.values()) == ["affine", "affine", "convex", "convex"]
    for name, per in fx["groups"].items():
        assert set(per) == set(fx["scores"]) and all(set(v) == {"0", "1", "2"} for v in per.values()), name
    # local alignment finds nothing for the later reads whatever the gaps: the first read's chain, as with linear gaps
    lin = next(g for g in load_fixture()["groups"] if g["name"] == "local_finds_nothing")["expected"]["0"]
    assert all(per["0"] == lin for per in fx["groups"]["local_finds_nothing"].values())
    # recompute the entries of every group of at most 20 000 bases x sequences (the large ones: on the generator's run only)
    small = [g["name"] for g in load_fixture()["groups"] if len(g["seqs"]) * sum(len(s) for s, _ in g["seqs"]) <= 20000]
    assert len(small) >= 18
    jobs = [(n, key, t) for n in small for key in fx["scores"] for t in (0, 1, 2)]
    with ProcessPoolExecutor(_workers()) as ex:
        for (name, key, t), e in ex.map(_gaps_job, jobs):
            assert fx["groups"][name][key][str(t)] == e, (name, key, t)
