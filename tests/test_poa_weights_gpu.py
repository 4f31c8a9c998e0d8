"""GPU suite (-m gpu): explicit weights and the consensus profile of POA groups (vc_poa_run_weighted) byte for byte against the
reference's fixture tests/golden/poa_weights.json.gz and against the restatement tests/poa_weights_ref.py."""
import os
import random

import numpy as np
import pytest

import poa_weights_cases as cases
import poa_weights_ref as W
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu
CASES = cases.cases()


def _gp(t, sc):
    return capi.VcPoaGapParams(device=0, algorithm=t, match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3], gap_open2=sc[4], gap_extend2=sc[5])


def _run(groups, weights, t, sc, strands=False, msa=False, graph=True, profile=True):
    x = poa._run(poa.group_batch(groups), _gp(t, sc), msa_flags=(capi.VC_POA_MSA | capi.VC_POA_MSA_CONSENSUS | capi.VC_POA_COVERAGE) if msa else (0 if graph or strands else None),
                 strands=strands, strand_scores=False, graph=graph, weights=poa.weight_arrays(groups, weights), profile=profile)
    assert all(int(s) == capi.VC_WIN_OK for s in x.status)
    return x


def _got(x, w, strands):
    pr = x.profiles[w]
    d = dict(consensus=x.cons[w], codes=pr.codes, counts=pr.counts.tolist(), edges=x.graphs[w].edges())
    if strands:
        d["reversed"] = x.msas[w].reversed
    return d


def _batches():
    """the fixture's entries with equal type, scores and strand flag go through one call"""
    by = {}
    for c in CASES:
        by.setdefault((c[3], c[4], c[5]), []).append(c)
    return sorted(by.items())


@pytest.mark.parametrize("key,entries", _batches(), ids=lambda v: "-".join(map(str, v[:2])) + ("-s" if v[2] else "") if isinstance(v, tuple) else None)
def test_fixture_byte_for_byte(built, key, entries):
    t, sc, strands = key
    x = _run([c[1] for c in entries], [c[2] for c in entries], t, sc, strands=strands)
    for w, c in enumerate(entries):
        cases.check(_got(x, w, strands), c[6], c[0])


def _random_groups(seed, n):
    rng = random.Random(seed)
    groups, weights = [], []
    for _ in range(n):
        base = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 120)))
        mem = []
        for _ in range(rng.randint(3, 12)):
            s = "".join(rng.choice("ACGT") if rng.random() < 0.04 else ch for ch in base if rng.random() > 0.03)
            q = bytes(33 + rng.randrange(3, 40) for _ in s) if rng.random() < 0.3 else None
            mem.append((s.encode(), q))
        groups.append(mem)
        weights.append(W.seeded_weights(mem, rng.randrange(1 << 30), "mix"))
    return groups, weights


@pytest.mark.parametrize("model,sc", (("linear", (5, -4, -8, -8, -8, -8)), ("affine", (5, -4, -8, -6, -8, -6)), ("convex", (5, -4, -8, -6, -10, -4))))
def test_300_seeded_groups_against_the_restatement(built, model, sc):
    groups, weights = _random_groups(77 + len(model), 300)
    for t in (0, 1, 2):
        sub = slice(t * 100, (t + 1) * 100)
        x = _run(groups[sub], weights[sub], t, sc, msa=True)
        for w, (mem, wt) in enumerate(zip(groups[sub], weights[sub])):
            r = W.run(mem, wt, t, *sc)
            got = _got(x, w, False)
            assert got["consensus"] == r["consensus"] and got["codes"] == r["codes"] and got["counts"] == r["counts"], (model, t, w)
            assert [tuple(e) for e in got["edges"]] == r["edges"], (model, t, w)
            m = x.msas[w]
            nc = len(got["codes"])
            assert [sum(got["counts"][k][j] for k in range(nc)) for j in range(len(got["consensus"]))] == m.coverage.tolist(), (model, t, w)   # (a)
            assert W.counts_from_rows(m.rows[:-1], m.rows[-1], got["codes"]) == got["counts"], (model, t, w)


def test_weight_one_is_the_plain_call_and_lut_weights_the_quality_call(built):
    groups, _ = _random_groups(5, 40)
    sc = (5, -4, -8, -8, -8, -8)
    plain = [[(s, None) for s, _ in g] for g in groups]
    a = poa.poa_graph(plain, "global")
    b = poa.poa_graph(plain, "global", weights=[[1] * len(g) for g in plain])
    withq = [[(s, bytes(33 + (i * 7 + k) % 40 for k in range(len(s)))) for i, (s, _) in enumerate(g)] for g in groups]
    lut = (np.ctypeslib.as_array((lambda t: (capi.load_hip().vc_weight_lut(t), t)[1])((capi.C.c_uint32 * 256)()))).tolist()
    c = poa.poa_graph(withq, "global")
    d = poa.poa_graph(plain, "global", weights=[[[lut[v] for v in q] for _, q in g] for g in withq])
    for u, v in ((a, b), (c, d)):
        for gu, gv in zip(u, v):
            assert gu.consensus == gv.consensus and gu.edges() == gv.edges() and gu.aligned_pairs() == gv.aligned_pairs() and gu.paths() == gv.paths()
            assert gu.node_base.tolist() == gv.node_base.tolist() and gu.rank_to_node.tolist() == gv.rank_to_node.tolist()


def test_no_weight_no_profile_is_the_selected_entry(built, capfd, monkeypatch):
    groups, _ = _random_groups(9, 30)
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    sc = (5, -4, -8, -6, -8, -6)
    batch = poa.group_batch(groups)
    zero = (np.zeros(sum(len(g) for g in groups), np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    outs = []
    for kw in (dict(), dict(weights=zero)):
        for req in (dict(), dict(msa_flags=capi.VC_POA_MSA | capi.VC_POA_COVERAGE), dict(msa_flags=0, strands=True), dict(msa_flags=capi.VC_POA_MSA, graph=True)):
            capfd.readouterr()
            x = poa._run(batch, _gp(1, sc), **req, **kw)
            log = capfd.readouterr().err
            outs.append((x.cons, [None if m is None else (m.rows, m.members) for m in x.msas or []], [g.edges() for g in x.graphs or []], log))
    assert outs[:4] == outs[4:]
    assert "profile" not in outs[0][3] and "done alignments" in outs[0][3]
    capfd.readouterr()
    x = poa._run(batch, _gp(1, sc), profile=True)
    assert "vc_large: profile launches=1 bytes=" in capfd.readouterr().err
    assert x.cons == outs[0][0]                          # the profile-only call's consensus is vc_poa_run_gaps's


def test_small_budgets_regrow_and_split_the_profile(built, capfd, monkeypatch):
    groups, weights = _random_groups(21, 1000)
    groups = [g[:4] for g in groups]
    weights = [w[:4] for w in weights]
    sc = (5, -4, -8, -8, -8, -8)
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    capfd.readouterr()
    ref = _run(groups, weights, 1, sc, graph=False)
    plain_log = capfd.readouterr().err
    monkeypatch.setenv("VC_LARGE_CAPS", "l:3,e:1")
    monkeypatch.setenv("VC_LARGE_MAT_MB", "0.25")
    x = _run(groups, weights, 1, sc, graph=False)
    log = capfd.readouterr().err
    assert "regrow" in log and "flags=labels" in log.replace("edges,", "")
    launches = [int(l.split("launches=")[1].split()[0]) for l in log.splitlines() if l.startswith("vc_large: profile")]
    assert launches and launches[0] > 1
    assert x.cons == ref.cons
    for a, b in zip(x.profiles, ref.profiles):
        assert a.codes == b.codes and a.counts.tolist() == b.counts.tolist()
    monkeypatch.delenv("VC_LARGE_CAPS"); monkeypatch.delenv("VC_LARGE_MAT_MB")
    capfd.readouterr()
    poa._run(poa.group_batch(groups), _gp(1, sc))
    base = capfd.readouterr().err
    n = lambda s: [l for l in s.splitlines() if "done alignments" in l][-1].split("alignments=")[1].split()[0]      # noqa: E731
    assert n(base) == n(plain_log)


def test_long_mode2_member_beside_mode0_members(built):
    rng = random.Random(4)
    base = "".join(rng.choice("ACGT") for _ in range(2000))
    mut = lambda: "".join(rng.choice("ACGT") if rng.random() < 0.02 else ch for ch in base).encode()      # noqa: E731
    g = [[(b"ACGTACGTAC", None), (b"ACGTTCGTAC", None)], [(mut(), None), (mut(), None), (mut(), None)], [(b"GGGTTT", None)]]
    wts = [[None, None], [None, [rng.randint(0, 9) for _ in range(2000)], None], [None]]
    x = _run(g, wts, 1, (5, -4, -8, -8, -8, -8))
    for w in range(3):
        r = W.run(g[w], wts[w], 1, 5, -4, -8)
        got = _got(x, w, False)
        assert got["consensus"] == r["consensus"] and got["counts"] == r["counts"] and [tuple(e) for e in got["edges"]] == r["edges"]


def _flip(groups, weights, seed):
    """every member reverse-complemented with probability 1/2 (its quality reversed); the weights stay as given: they belong to
    the member as it is passed, and the library reverses them where it keeps the reverse strand"""
    import poa_strand_ref as ps
    rng = random.Random(seed)
    out = []
    for g in groups:
        out.append([(ps.reverse_complement(s), None if q is None else q[::-1]) if rng.random() < 0.5 else (s, q) for s, q in g])
    return out, weights


@pytest.mark.parametrize("kind", ("base", "mix"))
def test_both_strands_against_the_restatement(built, kind):
    """fresh flipped groups with spoa's -s: kept reverse members carry reversed weights; compared with the restatement's -s loop, which
    adds the kept views with the weight list reversed.  poa_profile(strand_ambiguous=True) is the call with s and without o."""
    groups, _ = _random_groups(300 + len(kind), 60)
    groups, _ = _flip(groups, None, 17)
    weights = [W.seeded_weights(g, 500 + w, kind) for w, g in enumerate(groups)]
    sc = (5, -4, -8, -8, -8, -8)
    seen = 0
    for t, name in enumerate(("local", "global", "semi-global")):
        sub = slice(t * 20, (t + 1) * 20)
        x = _run(groups[sub], weights[sub], t, sc, strands=True)
        pr = poa.poa_profile(groups[sub], t, weights=weights[sub], strand_ambiguous=True)
        for w, (mem, wt) in enumerate(zip(groups[sub], weights[sub])):
            r = W.run(mem, wt, t, *sc, strands=True)
            got = _got(x, w, True)
            assert got["reversed"].tolist() == [bool(v) for v in r["reversed"]], (kind, t, w)
            assert got["consensus"] == r["consensus"] and got["codes"] == r["codes"] and got["counts"] == r["counts"], (kind, t, w)
            assert [tuple(e) for e in got["edges"]] == r["edges"], (kind, t, w)
            assert (pr[w].consensus, pr[w].codes, pr[w].counts.tolist()) == (r["consensus"], r["codes"], r["counts"]), (kind, t, w)
            seen += sum(1 for v, k in zip(r["reversed"], wt) if v and isinstance(k, list))
    assert seen >= 30, seen                              # kept reverse members with per-base weights


def test_refused_groups_beside_good_ones(built, monkeypatch):
    """No input of testable size makes the reference throw on a POA group (VC_WIN_INVALID), as tests/test_poa_strand_gpu.py and
    tests/test_poa_msa_gpu.py note, so the not-computed group is one the arena budget refuses (VC_WIN_OVERFLOW): n_codes = 0 and
    an empty block for it, with and without rows, graph and strands beside the profile; the neighbours as without it."""
    rng = random.Random(12)
    base = "".join(rng.choice("ACGT") for _ in range(3000))
    big = [("".join(rng.choice("ACGT") if rng.random() < 0.03 else ch for ch in base).encode(), None) for _ in range(24)]
    small, wts = _random_groups(31, 4)
    groups = [small[0], big, small[1], [], small[2], big, small[3]]
    weights = [wts[0], [3] * 24, wts[1], [], wts[2], None, wts[3]]
    sc = (5, -4, -8, -8, -8, -8)
    good = _run([g for g in groups if g is not big], [w for g, w in zip(groups, weights) if g is not big], 1, sc, msa=True)
    lib, C = capi.load_hip(), capi.C
    monkeypatch.setenv("VC_LARGE_ARENA_MB", "4")
    with pytest.raises(poa.PoaError) as ex:
        poa.poa_profile(groups, weights=weights)
    assert ex.value.groups == {1: capi.VC_WIN_OVERFLOW, 5: capi.VC_WIN_OVERFLOW}
    pr = poa.poa_profile(groups, weights=weights, strict=False)
    assert pr[1] is None and pr[5] is None
    for req in (dict(msa_flags=None, graph=False), dict(msa_flags=capi.VC_POA_MSA | capi.VC_POA_MSA_CONSENSUS | capi.VC_POA_COVERAGE, graph=True),
                dict(msa_flags=0, graph=False, strands=True, strand_scores=False)):
        x = poa._run(poa.group_batch(groups), _gp(1, sc), weights=poa.weight_arrays(groups, weights), profile=True, **req)
        assert [int(v) for v in x.status] == [0, capi.VC_WIN_OVERFLOW, 0, 0, 0, capi.VC_WIN_OVERFLOW, 0]
        for w in (1, 5):
            p = x.profiles[w]
            assert p.status == capi.VC_WIN_OVERFLOW and p.codes == b"" and p.consensus == b"" and p.counts.shape == (1, 0)
        assert x.profiles[3].codes == b"" and x.profiles[3].counts.shape == (1, 0) and x.profiles[3].status == capi.VC_WIN_OK
        if "strands" not in req:
            for k, w in enumerate((0, 2, 3, 4, 6)):
                a, b = x.profiles[w], good.profiles[k]
                assert (a.consensus, a.codes, a.counts.tolist()) == (b.consensus, b.codes, b.counts.tolist()), w
    # the tables themselves: n_codes 0 and a block of no entry for the refused groups
    batch = poa.group_batch(groups)
    cons, off, status, r, vb = poa._result_buffers(batch)
    po = capi.VcPoaProfileOut()
    assert lib.vc_poa_run_weighted(C.byref(_gp(1, sc)), None, C.byref(vb), C.byref(r), None, None, None, C.byref(po)) == 0
    nc = [len(good.profiles[0].codes), 0, len(good.profiles[1].codes), 0, len(good.profiles[3].codes), 0, len(good.profiles[4].codes)]
    assert po.n_groups == 7 and [po.n_codes[w] for w in range(7)] == nc and all(nc[w] for w in (0, 2, 4, 6))
    for w in (1, 3, 5):
        assert po.code_off[w] == po.code_off[w + 1] and po.prof_off[w] == po.prof_off[w + 1]
    assert int(status[1]) == int(status[5]) == capi.VC_WIN_OVERFLOW and off[1] == off[2] and off[5] == off[6]
    assert po.prof_off[6] == sum((nc[w] + 1) * (int(off[w + 1]) - int(off[w])) for w in range(6) if nc[w])


def test_degenerate_groups_beside_good_ones(built):
    g = [[(b"ACGTACGT", None), (b"ACGAACGT", None)], [], [(b"", None), (b"", None)], [(b"TTTT", None)]]
    pr = poa.poa_profile(g, weights=[[2, None], [], [None, 5], None])
    assert pr[1].codes == b"" and pr[1].counts.shape == (1, 0) and pr[2].codes == b"" and pr[2].consensus == b""
    assert pr[0].consensus == b"ACGTACGT" and pr[0].counts.shape == (5, 8) and pr[3].counts.tolist() == [[4 * 0 + 1] * 4, [0] * 4]
    m = poa.poa_msa(g, profile=True)
    assert m[0].profile.counts.tolist() == poa.poa_profile(g)[0].counts.tolist()


def test_command_line(built, tmp_path, capsys):
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_bytes(b">r1\nACGTACGTAC\n>r2\nACGTTCGTAC\n>r3\nACGTTCGTAC\n")
    b.write_bytes(b">x\nGGGTTTAAA\n>y\nGGGTTAAA\n")
    wf, pf = tmp_path / "w.tsv", tmp_path / "p.tsv"
    wf.write_bytes(b"%s\tr1\t10\n%s\ty\t1,1,1,1,1,1,1,1\n" % (str(a).encode(), str(b).encode()))
    assert poa.main(["-l", "1", "--weights", str(wf), "--profile", str(pf), str(a), str(b)]) == 0
    out = capsys.readouterr().out
    groups = [[(b"ACGTACGTAC", None), (b"ACGTTCGTAC", None), (b"ACGTTCGTAC", None)], [(b"GGGTTTAAA", None), (b"GGGTTAAA", None)]]
    pr = poa.poa_profile(groups, "global", weights=[[10, None, None], [None, [1] * 8]])
    assert pf.read_bytes() == poa.profile_tsv([str(a), str(b)], pr)
    assert out == "".join(">Consensus LN:i:%d\n%s\n" % (len(p.consensus), p.consensus.decode()) for p in pr)
    assert pr[0].consensus == b"ACGTACGTAC"
    # the other outputs beside --weights / --profile: -r 2 and --gfa go through the same one call
    pf2 = tmp_path / "p2.tsv"
    assert poa.main(["-l", "1", "-r", "2", "--weights", str(wf), "--profile", str(pf2), str(a), str(b)]) == 0
    out = capsys.readouterr().out
    m = poa.poa_msa(groups, "global", include_consensus=True, weights=[[10, None, None], [None, [1] * 8]])
    names = [[b"r1", b"r2", b"r3", b"Consensus"], [b"x", b"y", b"Consensus"]]
    assert out.encode() == b"".join(b">%s\n%s\n" % (n, row) for mm, nn in zip(m, names) for n, row in zip(nn, mm.rows))
    assert pf2.read_bytes() == pf.read_bytes() and m[0].rows[-1] == b"ACGTACGTAC"
    assert poa.main(["-l", "1", "--gfa", "--both-strands", "--weights", str(wf), "--profile", str(pf2), str(a), str(b)]) == 0
    out = capsys.readouterr().out
    g = poa.poa_graph(groups, "global", strand_ambiguous=True, weights=[[10, None, None], [None, [1] * 8]])
    assert out.encode() == g[0].to_gfa([b"r1", b"r2", b"r3"]) + g[1].to_gfa([b"x", b"y"])
    assert b"ew:f:20" in out.encode() and pf2.read_bytes() == pf.read_bytes()
