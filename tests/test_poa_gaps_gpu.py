"""GPU suite (-m gpu): affine and convex gaps for the POA-group consensus (vc_poa_run_gaps) byte for byte -- spoa's 18 known
answers, the seeded groups of poa_gaps_groups.json.gz (all three algorithms, two affine and two convex score sets), linear
parameter sets against vc_poa_run, the matrix budget with the planes counted, and the command line.  Each test prints its time."""
import os
import re
import subprocess
import sys
import time

import pytest

import fixtures
import poa_gaps_ref as R
from test_poa import load_fixture, members
from test_poa_gaps import load_gaps_fixture, load_kats
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALG = {"SW": 0, "NW": 1, "OV": 2}


def _gap_params(t, m, n, g, e, q, c):
    return capi.VcPoaGapParams(device=0, algorithm=t, match=m, mismatch=n, gap_open=g, gap_extend=e, gap_open2=q, gap_extend2=c)


# ------------------------------------------------------------------ 1. spoa's 18 known answers
def test_spoa_known_answers_with_gaps(built):
    t0 = time.time()
    seqs, quals = fixtures.load_sample_reads()
    kats = load_kats()
    n = 0
    for name, k in kats.items():
        g = [(s, q if k["quality"] else None) for s, q in zip(seqs, quals)]
        cons, status = poa.run_batch(poa.group_batch([g]), _gap_params(ALG[k["type"]], k["m"], k["n"], k["g"], k["e"], k["q"], k["c"]))
        assert int(status[0]) == capi.VC_WIN_OK and cons[0].decode() == k["consensus"], name
        n += 1
    # and through the keywords of poa_consensus
    k = kats["GlobalConvexWithQualities"]
    got = poa.poa_consensus([list(zip(seqs, quals))], "global", 5, -4, -8, gap_extend=-6, gap_open2=-10, gap_extend2=-2)
    assert got[0].decode() == k["consensus"]
    print(f"[spoa KATs, all subtypes] {n} byte-identical through vc_poa_run_gaps in {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. seeded groups against the restatement
@pytest.mark.parametrize("t", [0, 1, 2])
def test_seeded_groups_with_gaps(built, t):
    t0 = time.time()
    fx = load_gaps_fixture()
    groups = load_fixture()["groups"]
    n = 0
    for key, scores in fx["scores"].items():
        cons, status = poa.run_batch(poa.group_batch([members(g) for g in groups]), _gap_params(t, *scores))
        for g, c, s in zip(groups, cons, status):
            e = fx["groups"][g["name"]][key][str(t)]
            assert int(s) == e["status"], (key, g["name"], int(s))
            assert c.decode() == e["consensus"], (key, g["name"], len(c), len(e["consensus"]))
            n += 1
    print(f"[seeded groups, algorithm {t}] {n} byte-identical in {len(fx['scores'])} calls, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 3. linear parameter sets: what vc_poa_run computes
def test_linear_parameter_sets_equal_vc_poa_run(built):
    t0 = time.time()
    groups = [g for g in load_fixture()["groups"] if tuple(g["scores"]) == (5, -4, -8) and len(g["seqs"]) <= 17]
    batch = poa.group_batch([members(g) for g in groups])
    for t in (0, 1, 2):
        want = poa.run_batch(batch, capi.VcPoaParams(device=0, algorithm=t, match=5, mismatch=-4, gap=-8))
        for gaps in ((-8, -8, -8, -8), (-8, -10, -8, -10), (-8, -8, -12, -1), (-8, -9, -3, -9)):
            assert poa.gap_model(*gaps)[0] == "linear"
            got = poa.run_batch(batch, _gap_params(t, 5, -4, *gaps))
            assert got[0] == want[0] and got[1].tolist() == want[1].tolist(), (t, gaps)
    print(f"[linear sets] {len(groups)} groups x 3 algorithms x 4 sets equal vc_poa_run, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. the matrix budget counts planes
def _events(err):
    return [l[len("vc_large: "):] for l in err.splitlines() if l.startswith("vc_large: ")]


def test_matrix_budget_counts_planes(built, monkeypatch, capfd):
    """Two groups of two 100-base reads: each step aligns one 101 x 101 matrix per group, 40 804 bytes a plane.  Under 0.3 MiB
    the linear (1 plane) and affine (3) pair fits one launch, the convex (5) pair does not; under 0.15 MiB a convex matrix is
    above the budget alone and still runs.  The done line counts cells, not planes."""
    import random
    rng = random.Random(99)
    truth = [bytes(rng.choice(b"ACGT") for _ in range(100)) for _ in range(2)]
    groups = [[(t, None), (t[:40] + t[41:70] + b"GA" + t[70:], None)] for t in truth]
    groups = [[(s[:100], q) for s, q in g] for g in groups]
    sets = {"linear": (-8, -8, -8, -8), "affine": (-8, -6, -8, -6), "convex": (-8, -6, -10, -2)}
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    t0 = time.time()
    seen = {}
    try:
        for mb in ("0.3", "0.15"):
            monkeypatch.setenv("VC_LARGE_MAT_MB", mb)
            for kind, (g, e, q, c) in sets.items():
                capfd.readouterr()
                got = poa.poa_consensus(groups, "global", 5, -4, g, gap_extend=e, gap_open2=q, gap_extend2=c)
                ev = _events(capfd.readouterr().err)
                for k, grp in enumerate(groups):
                    assert got[k] == R.consensus(grp, 1, 5, -4, g, e, q, c), (mb, kind, k)
                steps = [tuple(int(x) for x in re.findall(r"=(\d+)", l)) for l in ev if l.startswith("step ")]
                done = [l for l in ev if l.startswith("done ")]
                assert done == ["done alignments=2 cells=20000"], (mb, kind, done)
                seen[mb, kind] = steps
    finally:
        for k in ("VC_LARGE_MAT_MB", "VC_LARGE_LOG"):
            monkeypatch.delenv(k)
    assert seen["0.3", "linear"] == [] and seen["0.3", "affine"] == [] and seen["0.3", "convex"] == [(2, 0)], seen
    assert seen["0.15", "linear"] == [] and seen["0.15", "affine"] == [(2, 0)] and seen["0.15", "convex"] == [(2, 2)], seen
    print(f"[matrix budget] step events {seen}, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. the command line
def test_command_line_gap_options_on_the_sample(built):
    sample = os.path.join(GOLDEN, "sample.fastq.gz")
    kats = load_kats()
    t0 = time.time()
    runs = (
        (["-l", "1", "--gap-extend", "-6"], "GlobalAffineWithQualities"),
        (["-l", "1", "--gap-extend", "-6", "--gap-open2", "-10", "--gap-extend2", "-2"], "GlobalConvexWithQualities"),
        (["-l", "0", "--gap-extend", "-6", "--gap-open2", "-10", "--gap-extend2", "-2"], "LocalConvexWithQualities"),
        (["-l", "2", "--gap-extend", "-6"], "SemiGlobalAffineWithQualities"),
    )
    for argv, name in runs:
        p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", *argv, sample], cwd=ROOT, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()
        c = kats[name]["consensus"]
        assert p.stdout.decode() == f">Consensus LN:i:{len(c)}\n{c}\n", name
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "--gap-extend", "1", sample], cwd=ROOT, capture_output=True, timeout=300)
    assert p.returncode == 1 and b"extension" in p.stderr
    print(f"[command line] {len(runs)} runs on the sample, {time.time() - t0:.1f} s")
