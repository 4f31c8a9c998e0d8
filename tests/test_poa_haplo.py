"""CPU suite of the haplotype split of POA groups (vc_poa_run_haplotypes, poa.poa_haplotypes): the restatement
tests/poa_haplo_ref.py gives the hand answers of tests/poa_haplo_cases.py and, where nothing is split, spoa's own consensus on the
committed fixtures; the argument checks come before the device in the header's order; the text writers; and the recall of the
rule on simulated reads of two haplotypes, whose counts are written to profiles/poa_haplo_recall.txt and asserted as floors."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import poa_haplo_cases as HC
import poa_haplo_ref as H
from test_poa import load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(case):
    name, mem, t, scores, rule, exp = case
    return H.haplotypes(mem, t, *scores, **rule)


@pytest.mark.parametrize("case", HC.CASES, ids=[c[0] for c in HC.CASES])
def test_restatement_gives_the_hand_answers(case):
    got, exp = _ref(case), case[5]
    for key, want in exp.items():
        assert got[key] == want, (case[0], key, got[key], want)
    assert sum(got["sizes"]) == sum(1 for s, _ in case[1] if len(s))
    if len(got["sizes"]) == 1:                                             # K = 1: nothing is removed, so haplotype 0 is the group's consensus
        assert got["haps"][0] == got["consensus"], case[0]


def test_cases_reach_the_edges_they_name():
    by = {c[0]: c for c in HC.CASES}
    # the round: with one round the member stays where the seeds' profiles put it
    c = by["a round changes an assignment"]
    one = H.haplotypes(c[1], c[2], *c[3], rounds=1)["members"]
    assert one == [0, 0, 0, 0, 1, 1, 1, 0] and _ref(c)["members"] == [0, 0, 0, 0, 1, 1, 1, 1]
    # the qualities: without them haplotype 0 takes the branch two reads walk
    c = by["qualities decide the branch"]
    plain = H.haplotypes([(s, None) for s, _ in c[1]], c[2], *c[3])
    assert plain["haps"][0] == HC.R and _ref(c)["haps"][0] == HC.sub(HC.R, 15, ord("T"))
    # the dissolved cluster existed: without the size rule the lone read keeps a haplotype of its own
    c = by["small cluster dissolved"]
    assert H.haplotypes(c[1], c[2], *c[3], max_haplotypes=4, min_reads=1)["sizes"] == [3, 3, 2, 1]
    c = by["every cluster below min_reads"]
    assert H.haplotypes(c[1], c[2], *c[3], max_haplotypes=4, min_reads=2)["sizes"] == [2, 2, 2, 2]


def test_fixture_groups_without_a_split_give_spoas_consensus():
    fx = load_fixture()
    n = single = 0
    for g in fx["groups"]:
        mem = members(g)
        for t, e in g["expected"].items():
            if e["status"] != 0:
                continue
            gr, weights = H.build(mem, int(t), *g["scores"])                 # one build serves both rules
            _, of, sizes = H.split(gr, **{**H.DEFAULTS, "max_haplotypes": 1})
            assert sizes == [sum(1 for s, _ in mem if len(s))] and H.hap_consensus(gr, weights, of, 0) == e["consensus"].encode(), (g["name"], t)
            _, of, sizes = H.split(gr, **H.DEFAULTS)
            if len(sizes) == 1:
                assert H.hap_consensus(gr, weights, of, 0) == e["consensus"].encode(), (g["name"], t)
                single += 1
            n += 1
    assert n and single
    print(f"[fixture] {n} entries: haplotype 0 of max_haplotypes = 1 is spoa's consensus; {single} single-haplotype groups with the defaults too")


# ------------------------------------------------------------------ the argument checks
def _call(lib, p, h, b, o=True, **override):
    cons = np.zeros(max(int(b.bases.size), 1), np.uint8)
    off = np.zeros(b.n_windows + 1, np.uint64)
    status = np.zeros(max(b.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = b.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in override.items():
        setattr(vb, k, v)
    out = capi.VcPoaHapOut()
    rc = lib.vc_poa_run_haplotypes(None if p is None else C.byref(p), None if h is None else C.byref(h), C.byref(vb), C.byref(r),
                                   C.byref(out) if o else None)
    return rc, lib.vc_poa_last_error().decode()


def _gp(**kw):
    p = capi.VcPoaGapParams(0, 1, 5, -4, -8, -8, -8, -8)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _hp(**kw):
    h = capi.VcPoaHapParams(2, 2, 250, 4, 0)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_entry_and_defaults(built):
    lib = capi.load_hip()
    h = capi.VcPoaHapParams()
    lib.vc_poa_hap_default_params(C.byref(h))
    assert (h.max_haplotypes, h.min_reads, h.min_permille, h.rounds, h.flags) == (2, 2, 250, 4, 0)
    assert C.sizeof(capi.VcPoaHapParams) == 20
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_haplotypes" in hdr and "VC_POA_HAP_MAX" in hdr


def test_argument_errors_come_before_the_device_in_order(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    bad_batch = dict(win_seq_off=None)
    # each call breaks the rule it names and every later one: the message must be the earlier rule's
    steps = [
        ("null", lambda: _call(lib, None, _hp(max_haplotypes=0), b, **bad_batch), "null argument"),
        ("null", lambda: _call(lib, _gp(algorithm=5), None, b, **bad_batch), "null argument"),
        ("null", lambda: _call(lib, _gp(algorithm=5), _hp(), b, o=False, **bad_batch), "null argument"),
        ("gaps", lambda: _call(lib, _gp(algorithm=5), _hp(max_haplotypes=0), b, **bad_batch), "algorithm"),
        ("gaps", lambda: _call(lib, _gp(match=128), _hp(max_haplotypes=0), b, **bad_batch), "scores"),
        ("h", lambda: _call(lib, _gp(), _hp(max_haplotypes=0, min_reads=0), b, **bad_batch), "max_haplotypes"),
        ("h", lambda: _call(lib, _gp(), _hp(max_haplotypes=9, min_reads=0), b, **bad_batch), "max_haplotypes"),
        ("h", lambda: _call(lib, _gp(), _hp(min_reads=0, min_permille=1001), b, **bad_batch), "min_reads"),
        ("h", lambda: _call(lib, _gp(), _hp(min_permille=1001, rounds=0), b, **bad_batch), "min_permille"),
        ("h", lambda: _call(lib, _gp(), _hp(rounds=0, flags=2), b, **bad_batch), "rounds"),
        ("h", lambda: _call(lib, _gp(), _hp(flags=2), b, **bad_batch), "flag"),
        ("batch", lambda: _call(lib, _gp(), _hp(), b, **bad_batch), "null array in batch"),
    ]
    for what, f, word in steps:
        rc, msg = f()
        assert rc == capi.VC_ERR_ARG and word in msg, (what, word, rc, msg)
    rc, msg = _call(lib, _gp(), _hp(max_haplotypes=8, min_permille=0, flags=1), b)
    assert rc in (capi.VC_OK, capi.VC_ERR_NO_DEVICE), msg


def test_python_parameters():
    h = poa.hap_params(3, 4, 0.1234, True, 2)
    assert (h.max_haplotypes, h.min_reads, h.min_permille, h.rounds, h.flags) == (3, 4, 123, 2, capi.VC_POA_HAP_INDELS)
    assert poa.hap_params(min_fraction=0.0005).min_permille == 0 and poa.hap_params(min_fraction=0.0015).min_permille == 2
    for kw in (dict(max_haplotypes=0), dict(max_haplotypes=9), dict(min_reads=0), dict(rounds=0), dict(min_fraction=-0.1),
               dict(min_fraction=1.5), dict(min_reads=True), dict(min_fraction=float("nan"))):
        with pytest.raises(ValueError):
            poa.hap_params(**kw)


def test_text_writers():
    a = poa.Haplotypes([b"ACGT", b"ACCT"], [3, 2], [0, 0, None, 1, 1, 0], [(2, b"G", b"C", 3, 2), (7, b"A", b"-", 3, 2)], 0)
    recs = [[(b"r%d" % k, b"", None) for k in range(6)], []]
    names = [b"x.fa", b"y.fa"]
    assert poa.haplotype_fasta(names, [a, None]) == b">x.fa_hap0 members=3\nACGT\n>x.fa_hap1 members=2\nACCT\n"
    assert poa.haplotype_members_tsv(names, recs, [a, None]) == b"x.fa\tr0\t0\nx.fa\tr1\t0\nx.fa\tr2\t-\nx.fa\tr3\t1\nx.fa\tr4\t1\nx.fa\tr5\t0\n"
    assert poa.haplotype_sites_tsv(names, [a, None]) == b"x.fa\t2\tG\tC\t3\t2\nx.fa\t7\tA\t-\t3\t2\n"


def test_command_line_parsing(tmp_path, capsys):
    a = poa.parse_args(["x.fa"])
    assert (a.haplotypes, a.hap_members, a.hap_sites, a.max_haplotypes, a.hap_min_reads, a.hap_min_fraction, a.hap_indels) == \
        (None, None, None, 2, 2, 0.25, False)
    a = poa.parse_args(["--haplotypes", "h.fa", "--hap-members", "m.tsv", "--hap-sites", "s.tsv", "--max-haplotypes", "3", "--hap-min-reads", "4",
                        "--hap-min-fraction", "0.1", "--hap-indels", "-l", "1", "x.fa", "y.fq"])
    assert (a.haplotypes, a.hap_members, a.hap_sites, a.max_haplotypes, a.hap_min_reads, a.hap_min_fraction, a.hap_indels, a.files) == \
        ("h.fa", "m.tsv", "s.tsv", 3, 4, 0.1, True, ["x.fa", "y.fq"])
    for argv in (["--max-haplotypes", "two", "x.fa"], ["--hap-min-fraction", "x", "x.fa"], ["--hap-min-reads", "1.5", "x.fa"], ["--haplotypes"]):
        with pytest.raises(SystemExit):
            poa.parse_args(argv)
    # the haplotype outputs go with the plain consensus only, and their parameters are checked: exit 1 before any file is written
    fa = tmp_path / "g.fa"
    fa.write_text(">a\nACGT\n>b\nACGT\n")
    out = tmp_path / "h.fa"
    for extra in (["-r", "1"], ["--coverage"], ["--gfa"], ["--both-strands"], ["--correct", str(tmp_path / "c.fa")],
                  ["--profile", str(tmp_path / "p.tsv")], ["--save-graphs", str(tmp_path / "g.npz")],
                  ["--align", str(fa), "--align-out", str(tmp_path / "a.tsv")]):
        assert poa.main(["--haplotypes", str(out)] + extra + [str(fa)]) == 1, extra
        assert "--haplotypes" in capsys.readouterr().err
    for extra, word in ((["--max-haplotypes", "9"], "max_haplotypes"), (["--hap-min-reads", "0"], "min_reads"), (["--hap-min-fraction", "1.5"], "min_fraction")):
        assert poa.main(["--hap-sites", str(out)] + extra + [str(fa)]) == 1, extra
        assert word in capsys.readouterr().err
    assert not out.exists()


# ------------------------------------------------------------------ simulated recall
def _edit(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[-1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def _simulate(noise):
    rng = random.Random(20251)
    h0 = bytes(rng.choice(b"ACGT") for _ in range(400))
    planted = [40, 130, 215, 300, 370]
    h1 = bytearray(h0)
    for p in planted:
        h1[p] = rng.choice([c for c in b"ACGT" if c != h0[p]])
    h1 = bytes(h1)
    reads, truth = [], []
    for k in range(30):
        src = (h0, h1)[k % 2]
        out = bytearray()
        for ch in src:
            x = rng.random()
            if x < noise / 3:
                continue                                                   # deletion
            out.append(rng.choice(b"ACGT") if x < 2 * noise / 3 else ch)   # substitution
            if 2 * noise / 3 <= x < noise:
                out.append(rng.choice(b"ACGT"))                            # insertion
        reads.append((bytes(out), None))
        truth.append(k % 2)
    return h0, h1, planted, reads, truth


def test_error_free_reads_are_split_exactly():
    h0, h1, planted, reads, truth = _simulate(0.0)
    got = H.haplotypes(reads, 1, 5, -4, -8)
    assert got["haps"] == [h0, h1] and got["members"] == truth and got["sizes"] == [15, 15]
    assert [s[0] for s in got["sites"]] == planted


def test_noisy_reads_recall_floors():
    """8 % read errors, depth 30, the restatement on the CPU against the simulated truth.  The floors are the counts this test
    measured (profiles/poa_haplo_recall.txt): the rule is deterministic, so they hold until the rule changes."""
    h0, h1, planted, reads, truth = _simulate(0.08)
    got = H.haplotypes(reads, 1, 5, -4, -8)
    assert len(got["sizes"]) == 2
    flip = sum(a == b for a, b in zip(got["members"], truth)) < 15
    right = sum((a == b) != flip for a, b in zip(got["members"], truth))
    d = sorted(_edit(got["haps"][k], (h1, h0)[k] if flip else (h0, h1)[k]) for k in range(2))
    # a planted site is found where a site's alleles are the two planted bases
    want = {(min(h0[p], h1[p]), max(h0[p], h1[p])) for p in planted}
    found = sum((min(a, b), max(a, b)) in want for _, a, b, _, _ in got["sites"])
    text = (f"haplotype recall of the rule's restatement (tests/test_poa_haplo.py::test_noisy_reads_recall_floors)\n"
            f"two haplotypes of 400 bases, {len(planted)} planted SNPs, depth 30, 8 % read errors, seed 20251, defaults\n"
            f"members placed right: {right} / 30\nhaplotype consensus edit distance to truth: {d[0]} and {d[1]}\n"
            f"sites found: {len(got['sites'])}, of which with a planted pair of alleles: {found} (planted: {len(planted)})\n")
    print(text)
    if os.environ.get("VC_WRITE_PROFILES") == "1":
        open(os.path.join(ROOT, "profiles", "poa_haplo_recall.txt"), "w").write(text)
    assert right >= FLOOR_RIGHT and d[1] <= FLOOR_EDIT and found >= FLOOR_FOUND


FLOOR_RIGHT, FLOOR_EDIT, FLOOR_FOUND = 30, 0, 4          # as measured: profiles/poa_haplo_recall.txt
