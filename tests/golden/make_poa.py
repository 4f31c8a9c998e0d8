"""Generates tests/golden/poa_groups.json.gz: known answers for the POA-group consensus (vc_poa_run, vechat_amd/poa.py) from the REAL
reference.  Runs where oracle/_ref was built (after build()): every expected consensus comes from spoa itself, through the harness
entry vcref_spoa_consensus of oracle/_ref/libvcref_sse41.so (spoa's SIMD engine, the build the reference ships), and the scalar
build libvcref_sisd.so must agree on every entry.

  python tests/golden/make_poa.py

Records:
  kat     the semi-global (kOV) counterparts of spoa's four known-answer tests: the 55 reads of sample.fastq.gz at 5/-4/-8, with and
          without qualities (spoa_kat.json holds the local and global ones);
  groups  seeded groups, their sequences stored here, each with the expected status and consensus of all three algorithms at its
          scores: sizes 1, 2, 3, 17 and 64, lengths 1 to 1 200 (across k_lg_fwd's 512-column chunks), FASTA and FASTQ members,
          reverse-complemented members, partial reads, an N / IUPAC read, repeats, a group where local alignment finds nothing,
          empty sequences and an empty group;
  invalid the bad inputs and what each gives: an empty sequence and an empty group are accepted by the reference
          (nothing added; the empty consensus), a quality string of the wrong length makes it throw (graph.cpp:191-196) -- the
          batch format cannot carry one, so vechat_amd.poa refuses it before the device.
"""
import ctypes as C
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fixtures  # noqa: E402
import oracle_api as oa  # noqa: E402

SEED = 20261016
SCORES = (5, -4, -8)                                     # spoa's -m -n -g defaults and the known-answer tests' scores
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def ref_consensus(lib, members, atype, m, n, g):
    """members [(bytes, bytes | None)] -> (rc, consensus) from vcref_spoa_consensus (rc -1: the reference threw)"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    sa = SA(*[s for s, _ in members])
    qa = SA(*[q for _, q in members])
    la = (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members])
    cap = sum(len(s) for s, _ in members) + 16
    out = C.create_string_buffer(cap)
    out_len = C.c_uint32(0)
    rc = lib.vcref_spoa_consensus(C.c_uint32(k), sa, la, qa, C.c_int(atype), C.c_int(m), C.c_int(n), C.c_int(g), out,
                                  C.c_uint32(cap), C.byref(out_len))
    return rc, (out.raw[:out_len.value] if rc == 0 else b"")


def expected(members, scores):
    """{"0" / "1" / "2": {"status", "consensus"}} from the SIMD build, checked against the scalar one"""
    simd, sisd = oa.load_ref("sse41"), oa.load_ref("sisd")
    res = {}
    for t in (0, 1, 2):
        a, b = ref_consensus(simd, members, t, *scores), ref_consensus(sisd, members, t, *scores)
        assert a == b, ("the SIMD and scalar builds of the reference disagree", t, scores, [len(s) for s, _ in members])
        assert a[0] in (0, -1), a[0]
        res[str(t)] = dict(status=0 if a[0] == 0 else 4, consensus=a[1].decode())   # VC_WIN_OK / VC_WIN_INVALID
    return res


def revcomp(s):
    return s.translate(_COMP)[::-1]


def mutate(rng, s, rate, alphabet=b"ACGT"):
    """substitutions, insertions and deletions, each a third of `rate`"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))
        out.append(rng.choice([x for x in alphabet if x != c]) if rng.random() < rate / 3 else c)
    return bytes(out)


def qual(rng, n, lo=2, hi=40):
    return bytes(33 + rng.randint(lo, hi) for _ in range(n))


def members_of(rng, truth, size, rate=0.08, fastq=0.5, rc=0.0, partial=0.0, min_len=1):
    """`size` reads of `truth`: noisy copies, some reverse-complemented, some partial; FASTQ with probability `fastq`"""
    out = []
    for _ in range(size):
        s = truth
        if partial and rng.random() < partial and len(s) > 8:
            a = rng.randrange(0, len(s) // 2)
            b = rng.randrange(a + max(1, len(s) // 4), len(s) + 1)
            s = s[a:b]
        s = mutate(rng, s, rate) or s[:1]
        if len(s) < min_len:
            s = truth[:min_len]
        if rc and rng.random() < rc:
            s = revcomp(s)
        out.append((s, qual(rng, len(s)) if rng.random() < fastq else None))
    return out


def seeded_groups(rng):
    """[(name, members, scores)]"""
    R = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    G = []
    G.append(("size1_len1", [(b"G", None)], SCORES))
    G.append(("size1_len57_fastq", [(R(57), qual(rng, 57))], SCORES))
    G.append(("size2_len12_fasta", members_of(rng, R(12), 2, fastq=0.0), SCORES))
    G.append(("size2_len300_fastq", members_of(rng, R(300), 2, fastq=1.0), SCORES))
    G.append(("size3_len1_to_3", [(b"A", None), (b"AC", qual(rng, 2)), (b"TAC", None)], SCORES))
    G.append(("size3_len100_mixed", members_of(rng, R(100), 3), SCORES))
    G.append(("size3_len513", members_of(rng, R(513), 3, rate=0.05), SCORES))
    for L in (200, 511, 512, 1025, 1200):
        G.append((f"size17_len{L}", members_of(rng, R(L), 17, rate=0.10), SCORES))
    G.append(("size64_len120", members_of(rng, R(120), 64, rate=0.12), SCORES))
    G.append(("size64_len300_partial", members_of(rng, R(300), 64, rate=0.08, partial=0.4), SCORES))
    G.append(("size9_len1023_partial", members_of(rng, R(1023), 9, rate=0.06, partial=0.6), SCORES))
    G.append(("size12_len400_revcomp", members_of(rng, R(400), 12, rate=0.08, rc=0.4), SCORES))
    t = R(250)
    G.append(("size10_len250_revcomp_partial", members_of(rng, t, 10, rate=0.05, rc=0.3, partial=0.5), SCORES))
    iu = members_of(rng, R(180), 8, rate=0.06)
    s = bytearray(iu[3][0])
    for k in rng.sample(range(len(s)), 30):
        s[k] = rng.choice(b"NNNNRYSWKMBDHV")
    iu[3] = (bytes(s), iu[3][1] and qual(rng, len(s)))
    iu[5] = (b"N" * 40 + iu[5][0][40:], iu[5][1])
    G.append(("size8_len180_iupac", iu, SCORES))
    G.append(("local_finds_nothing", [(b"AAAAAAAAAA", None), (b"CCCCCCCCCC", qual(rng, 10)), (b"GGGGTTTT", None), (b"AAAAA", None)], SCORES))
    G.append(("homopolymers", [(b"A" * n, None if n % 2 else qual(rng, n)) for n in (30, 28, 31, 29, 30, 33, 1)], SCORES))
    G.append(("dinucleotide_repeats", [(b"AC" * 40, None), (b"CA" * 40, None), (b"AC" * 38 + b"A", None), (b"C" + b"AC" * 41, None),
                                      (b"AC" * 20, None)], SCORES))
    G.append(("low_qualities", [(s, bytes(33 + rng.randint(0, 3) for _ in s)) for s, _ in members_of(rng, R(90), 6)], SCORES))
    G.append(("empty_sequence_first", [(b"", None)] + members_of(rng, R(80), 4), SCORES))
    G.append(("empty_sequence_between", members_of(rng, R(80), 2) + [(b"", qual(rng, 0))] + members_of(rng, R(80), 2), SCORES))
    G.append(("empty_sequences_only", [(b"", None), (b"", None)], SCORES))
    G.append(("empty_group", [], SCORES))
    G.append(("scores_3_-5_-4", members_of(rng, R(300), 10, rate=0.1, partial=0.3), (3, -5, -4)))
    G.append(("scores_1_-1_-1_ties", members_of(rng, R(150), 8, rate=0.15), (1, -1, -1)))
    G.append(("scores_2_-3_0_free_gaps", members_of(rng, R(120), 6, rate=0.1), (2, -3, 0)))
    G.append(("scores_127_-128_-128", members_of(rng, R(200), 6, rate=0.1), (127, -128, -128)))
    return G


def main():
    rng = random.Random(SEED)
    seqs, quals = fixtures.load_sample_reads()
    simd = oa.load_ref("sse41")
    kat = {}
    for name, q in (("SemiGlobal", False), ("SemiGlobalWithQualities", True)):
        members = list(zip(seqs, quals if q else [None] * len(seqs)))
        e = expected(members, SCORES)["2"]
        assert e["status"] == 0
        kat[name] = dict(type="OV", m=SCORES[0], n=SCORES[1], g=SCORES[2], quality=q, consensus=e["consensus"])
    # the generator is pinned by the four committed known answers
    for name, k in fixtures.load_kats().items():
        members = list(zip(seqs, quals if k["quality"] else [None] * len(seqs)))
        assert ref_consensus(simd, members, {"SW": 0, "NW": 1}[k["type"]], k["m"], k["n"], k["g"]) == (0, k["consensus"].encode()), name
    groups = []
    for name, members, scores in seeded_groups(rng):
        groups.append(dict(name=name, scores=list(scores),
                           seqs=[[s.decode(), None if q is None else q.decode()] for s, q in members],
                           expected=expected(members, scores)))
    bad_q = [(b"ACGTACGT", None), (b"ACGTTCGT", b"IIII")]
    invalid = [
        dict(case="empty sequence", group="empty_sequence_between", expected="VC_WIN_OK: nothing added (graph.cpp:187-190)"),
        dict(case="group of empty sequences", group="empty_sequences_only", expected="VC_WIN_OK: the empty consensus"),
        dict(case="empty group", group="empty_group", expected="VC_WIN_OK: the empty consensus (graph.cpp:534-537)"),
        dict(case="quality string of the wrong length", seqs=[[s.decode(), None if q is None else q.decode()] for s, q in bad_q],
             expected="ValueError from vechat_amd.poa.group_batch; the reference throws (graph.cpp:191-196), and vc_batch cannot "
                      "carry it (qualities share the bases' offsets)"),
    ]
    fx = dict(params=dict(seed=SEED, m=SCORES[0], n=SCORES[1], g=SCORES[2], generator="tests/golden/make_poa.py",
                          reference="oracle/_ref/libvcref_sse41.so vcref_spoa_consensus, libvcref_sisd.so agreeing"),
              kat=kat, groups=groups, invalid=invalid)
    out = os.path.join(HERE, "poa_groups.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(groups), "groups,", sum(len(g["seqs"]) for g in groups), "sequences,",
          sum(len(s) for g in groups for s, _ in g["seqs"]), "bases")


if __name__ == "__main__":
    main()
