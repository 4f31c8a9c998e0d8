"""GPU suite (-m gpu): the haplotype split of POA groups on the device (vc_poa_run_haplotypes, poa.poa_haplotypes) against the
restatement tests/poa_haplo_ref.py, every output array compared: the hand-built cases of tests/poa_haplo_cases.py call by call
and all in one batch, the wave's tile boundaries (63, 64, 65 and 70 members, more than 64 and more than 128 columns, 66 sites),
a group whose tables regrow first, a refused group between good ones, and the Python entry end to end.  r is compared against
vc_poa_run_gaps everywhere.

No input of testable size makes the reference throw on a POA group (VC_WIN_INVALID), so the group that is not computed is one
the arena budget refuses (VC_WIN_OVERFLOW), as in tests/test_poa_graph_gpu.py."""
import random
import time

import pytest

import poa_haplo_cases as HC
import poa_haplo_ref as H
from vechat_amd import capi, poa

pytestmark = pytest.mark.gpu


def _rule(rule):
    r = {**H.DEFAULTS, **rule}
    return capi.VcPoaHapParams(r["max_haplotypes"], r["min_reads"], r["min_permille"], r["rounds"], capi.VC_POA_HAP_INDELS if r["indels"] else 0)


def _same(got, want, w):
    """a poa.Haplotypes against the restatement's dict of the same group, every array"""
    assert got.consensus == want["haps"] and got.sizes == want["sizes"], (w, got.consensus, want["haps"], got.sizes, want["sizes"])
    assert [capi.VC_POA_HAP_NONE if m is None else m for m in got.members] == want["members"], (w, got.members, want["members"])
    assert [(c, a[0], b[0], na, nb) for c, a, b, na, nb in got.sites] == want["sites"], (w, got.sites, want["sites"])


def _check(groups, t, scores, rule, refs=None):
    """one call on `groups`; every array against the restatement (refs: already computed), and r against vc_poa_run_gaps"""
    batch = poa.group_batch(groups)
    p = capi.VcPoaGapParams(0, t, *scores)
    cons, status, res, raw = poa.run_batch_haplotypes(batch, p, _rule(rule))
    plain, pstatus = poa.run_batch(batch, p)
    assert cons == plain and status.tolist() == pstatus.tolist() == [capi.VC_WIN_OK] * len(groups)
    refs = refs or [H.haplotypes(g, t, *scores, **rule) for g in groups]
    for w, (want, got) in enumerate(zip(refs, res)):
        assert cons[w] == want["consensus"], w
        _same(got, want, w)
    # the raw tables are prefix tables over the whole batch
    assert raw["n_haps"].tolist() == [len(x["sizes"]) for x in refs] and int(raw["hap_first"][-1]) == sum(len(x["sizes"]) for x in refs)
    assert int(raw["site_off"][-1]) == sum(len(x["sites"]) for x in refs) and raw["bytes"] > 0
    return res


@pytest.mark.parametrize("case", HC.CASES, ids=[c[0] for c in HC.CASES])
def test_every_case_against_the_restatement(built, case):
    name, mem, t, scores, rule, exp = case
    res = _check([mem], t, scores, rule)
    for key, attr in (("sizes", "sizes"), ("haps", "consensus")):           # and the hand answer itself
        if key in exp:
            assert getattr(res[0], attr) == exp[key], (name, key)


def test_all_cases_in_one_batch_with_mixed_haplotype_counts(built):
    t0 = time.time()
    groups = [c[1] for c in HC.CASES]
    rule = dict(max_haplotypes=3)
    refs = [H.haplotypes(g, 1, *HC.LINEAR, **rule) for g in groups]
    assert {len(x["sizes"]) for x in refs} >= {1, 2, 3}
    _check(groups, 1, HC.LINEAR, rule, refs)
    print(f"[one batch] {len(groups)} groups, haplotype counts {sorted(len(x['sizes']) for x in refs)}, {time.time() - t0:.1f} s")


def _two(n0, n1, L=20, step=None, seed=5, start=1):
    """n0 reads of a random L-base haplotype and n1 of one that differs at every step-th base from `start` (step None: at one base)"""
    rng = random.Random(seed)
    a = bytes(rng.choice(b"ACGT") for _ in range(L))
    b = bytearray(a)
    for p in (range(start, L, step) if step else [L // 2]):
        b[p] = rng.choice([c for c in b"ACGT" if c != a[p]])
    return [(a, None)] * n0 + [(bytes(b), None)] * n1


@pytest.mark.parametrize("S", [63, 64, 65, 70])
def test_member_tiles(built, S):
    groups = [_two(S - S // 3, S // 3, seed=S)]
    res = _check(groups, 1, HC.LINEAR, {})
    assert res[0].sizes == [S - S // 3, S // 3]


@pytest.mark.parametrize("L", [70, 140])
def test_column_tiles(built, L):
    res = _check([_two(3, 3, L=L, step=33, seed=L)], 1, HC.LINEAR, {})
    assert res[0].sizes == [3, 3] and [s[0] for s in res[0].sites] == list(range(1, L, 33))


def test_66_sites(built):
    res = _check([_two(3, 3, L=200, step=3, seed=66, start=2)], 1, HC.LINEAR, {})          # bases 2, 5, .. 197
    assert [s[0] for s in res[0].sites] == list(range(2, 200, 3)) and len(res[0].sites) == 66 and res[0].sizes == [3, 3]


def test_a_table_regrows_before_the_stage(built, monkeypatch, capfd):
    groups = [HC.fa(HC.H1, HC.H1, HC.H1, HC.H2, HC.H2, HC.H2, HC.H3, HC.H3, HC.H3), _two(4, 3, L=70, step=20)]
    monkeypatch.setenv("VC_LARGE_CAPS", "n:4,e:4,a:5,l:4,s:6,p:4")
    monkeypatch.setenv("VC_LARGE_LOG", "1")
    capfd.readouterr()
    _check(groups, 1, HC.LINEAR, dict(max_haplotypes=3))
    err = capfd.readouterr().err
    assert "vc_large: regrow" in err and "vc_large: haplotypes launches=" in err


def test_a_refused_group_between_good_ones(built, monkeypatch):
    """the neighbours of the group that is not computed give the restatement's arrays, as they do alone"""
    rng = random.Random(91)
    big = [(bytes(rng.choice(b"ACGT") for _ in range(3000)), None) for _ in range(24)]
    groups = [HC.fa(HC.H1, HC.H1, HC.H1, HC.H2, HC.H2, HC.H2, HC.H3, HC.H3, HC.H3), big, HC.fa(HC.R, HC.R, HC.R, HC.V9, HC.V9, HC.V9, HC.X9)]
    want = {w: H.haplotypes(groups[w], 1, *HC.LINEAR) for w in (0, 2)}
    monkeypatch.setenv("VC_LARGE_ARENA_MB", "4")
    batch, p = poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *HC.LINEAR)
    cons, status, res, raw = poa.run_batch_haplotypes(batch, p, _rule({}))
    plain, pstatus = poa.run_batch(batch, p)
    loose = poa.poa_haplotypes(groups, strict=False)
    with pytest.raises(poa.PoaError):
        poa.poa_haplotypes(groups)
    assert cons == plain and status.tolist() == pstatus.tolist() == [capi.VC_WIN_OK, capi.VC_WIN_OVERFLOW, capi.VC_WIN_OK]
    assert raw["n_haps"].tolist() == [len(want[0]["sizes"]), 0, len(want[2]["sizes"])]
    assert res[1].consensus == [] and res[1].sites == [] and res[1].members == [None] * 24 and cons[1] == b""
    for w in (0, 2):
        assert cons[w] == want[w]["consensus"]
        _same(res[w], want[w], w)
    assert loose[1] is None and loose[0].sizes == want[0]["sizes"]


def test_python_entry_and_command_line_end_to_end_on_two_files(built, tmp_path, capsysbinary):
    recs = [[(b"r%d" % k, s, q) for k, (s, q) in enumerate([(HC.R, None)] * 2 + [(HC.R, b"I" * 20)] + [(HC.V9, None)] * 3)],
            [(b"d%d" % k, s, None) for k, s in enumerate([HC.R, HC.R, HC.R, HC.D9, HC.D9, HC.D9])]]
    files = []
    for k, rs in enumerate(recs):
        f = tmp_path / f"g{k}.fq"
        # FASTQ for a record with a quality, FASTA for the rest: two files, one of each kind
        if k == 0:
            f.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, q if q is not None else b"5" * len(s)) for n, s, q in rs))
        else:
            f = tmp_path / f"g{k}.fa"
            f.write_bytes(b"".join(b">%s\n%s\n" % (n, s) for n, s, _ in rs))
        files.append(str(f))
    from vechat_amd import seqio
    groups = [[(data, qual) for _, data, qual in seqio.read_sequences(f)] for f in files]
    want = [H.haplotypes(g, 1, *HC.LINEAR, indels=True) for g in groups]
    got = poa.poa_haplotypes(groups, indels=True, algorithm="global")
    for w in range(2):
        _same(got[w], want[w], w)
        assert got[w].status == capi.VC_WIN_OK
    assert got[0].consensus == [HC.R, HC.V9] and got[1].consensus == [HC.R, HC.D9] and got[1].members == [0, 0, 0, 1, 1, 1]
    assert poa.poa_haplotypes(groups, max_haplotypes=1)[1].sizes == [6] and poa.poa_haplotypes([]) == []
    hf, mf, sf = (str(tmp_path / n) for n in ("h.fa", "m.tsv", "s.tsv"))
    capsysbinary.readouterr()
    assert poa.main(["-l", "1", "--haplotypes", hf, "--hap-members", mf, "--hap-sites", sf, "--hap-indels"] + files) == 0
    out = capsysbinary.readouterr().out
    assert out == b"".join(b">Consensus LN:i:%d\n%s\n" % (len(x["consensus"]), x["consensus"]) for x in want)
    names = [f.encode() for f in files]
    assert open(hf, "rb").read() == b"".join(b">%s_hap%d members=%d\n%s\n" % (n, k, x["sizes"][k], x["haps"][k])
                                             for n, x in zip(names, want) for k in range(len(x["sizes"])))
    assert open(mf, "rb").read() == b"".join(b"%s\t%s\t%s\n" % (n, r[0], b"-" if m == H.HAP_NONE else b"%d" % m)
                                             for n, rs, x in zip(names, recs, want) for r, m in zip(rs, x["members"]))
    assert open(sf, "rb").read() == b"".join(b"%s\t%d\t%c\t%c\t%d\t%d\n" % ((n,) + s) for n, x in zip(names, want) for s in x["sites"])
    # without the flag the second file holds one haplotype, and only the file asked for is written
    h2 = str(tmp_path / "h2.fa")
    assert poa.main(["-l", "1", "--haplotypes", h2, files[1]]) == 0
    assert open(h2, "rb").read() == b">%s_hap0 members=6\n%s\n" % (names[1], want[1]["consensus"])
