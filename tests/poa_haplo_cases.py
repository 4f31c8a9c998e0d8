"""TEST INFRASTRUCTURE: one hand-built group per edge of the haplotype rule (include/vechat_hip.h), for tests/test_poa_haplo.py
(the restatement gives the hand answers) and tests/test_poa_haplo_gpu.py (the device gives the restatement's arrays).

Every group is made of a 20-base backbone R and variants of it, aligned globally unless the case says otherwise, so that a
column is a position of R and the answers can be written down: R's bytes appear in the order A, C, G, T, which is the code
order that decides a tie between alleles.  A case is (name, members, algorithm, scores, rule, expected); expected holds what
was worked out by hand -- any of sizes, members, haps, sites -- and may be empty where only the device-against-restatement
comparison applies.

Not in this table: a group that is not computed between good ones.  No input of testable size makes the reference throw on a POA
group (VC_WIN_INVALID needs a worst-case score beyond int32), so, as in the earlier POA suites, that group is one the arena
budget refuses (VC_WIN_OVERFLOW): tests/test_poa_haplo_gpu.py::test_a_refused_group_between_good_ones puts it between two groups
of this table's members and compares the neighbours with the restatement.
"""
R = b"ACGTTGCAAGCTTAGGCATC"
LINEAR = (5, -4, -8, -8, -8, -8)
AFFINE = (5, -4, -8, -6, -8, -6)


def sub(s, pos, base):
    return s[:pos] + bytes([base]) + s[pos + 1:]


def fa(*seqs):
    return [(s, None) for s in seqs]


V9 = sub(R, 9, ord("C"))                                  # R[9] is G
X9 = sub(R, 9, ord("A"))                                  # a third base at the same site
D9 = R[:9] + R[10:]                                       # R without base 9 (its neighbours differ from it: the gap has one place)
# three haplotypes, each the odd one out at a site of its own: any two agree at one site and disagree at two
H1, H2, H3 = sub(R, 4, ord("A")), sub(R, 9, ord("C")), sub(R, 15, ord("T"))
HX = sub(sub(sub(R, 4, ord("A")), 9, ord("C")), 15, ord("T"))   # the minor allele at all three
# four haplotypes over the three 2 : 2 splits of {a, b, c, d}: every pair agrees at one site and disagrees at two
QA = R
QB = sub(sub(R, 9, ord("C")), 15, ord("T"))
QC = sub(sub(R, 4, ord("A")), 15, ord("T"))
QD = sub(sub(R, 4, ord("A")), 9, ord("C"))
# a seed that is half wrong: s0 carries the first three alleles of one haplotype and the fourth of the other
S4 = (2, 6, 11, 17)                                       # R there: G, C, T, A
PA = R
PB = sub(sub(sub(sub(R, 2, ord("A")), 6, ord("A")), 11, ord("A")), 17, ord("C"))
P0 = sub(R, 17, ord("C"))
PY = sub(sub(sub(sub(R, 2, ord("T")), 6, ord("T")), 11, ord("C")), 17, ord("C"))   # third bases at the first three sites
QLOW, QHIGH = b"#" * 20, b"I" * 20

CASES = [
    ("no site", fa(R, R, R, R), 1, LINEAR, {}, dict(sizes=[4], members=[0, 0, 0, 0], haps=[R], sites=[])),
    # 3 + 3: equal counts, the earlier code (C before G) is the major allele; equal sizes, the smaller label comes first
    ("one SNP 3 + 3", fa(R, R, R, V9, V9, V9), 1, LINEAR, {},
     dict(sizes=[3, 3], members=[0, 0, 0, 1, 1, 1], haps=[R, V9], sites=[(9, ord("C"), ord("G"), 3, 3)])),
    ("allele exactly at min_reads", fa(R, R, R, R, V9, V9), 1, LINEAR, {},
     dict(sizes=[4, 2], members=[0, 0, 0, 0, 1, 1], haps=[R, V9], sites=[(9, ord("G"), ord("C"), 4, 2)])),
    ("allele one read below min_reads", fa(R, R, R, R, R, V9), 1, LINEAR, {}, dict(sizes=[6], members=[0] * 6, haps=[R], sites=[])),
    # 1000 * 2 == 250 * 8
    ("permille exactly met", fa(R, R, R, R, R, R, V9, V9), 1, LINEAR, {},
     dict(sizes=[6, 2], members=[0] * 6 + [1, 1], haps=[R, V9], sites=[(9, ord("G"), ord("C"), 6, 2)])),
    # 1000 * 2 < 250 * 9
    ("permille one read below", fa(R, R, R, R, R, R, R, V9, V9), 1, LINEAR, {}, dict(sizes=[9], members=[0] * 9, haps=[R], sites=[])),
    # the third base votes 0 and joins the smallest k; with max_haplotypes 3 its d is 0, so it must not seed
    ("third base votes 0", fa(R, R, R, V9, V9, V9, X9), 1, LINEAR, {},
     dict(sizes=[4, 3], members=[0, 0, 0, 1, 1, 1, 0], haps=[R, V9], sites=[(9, ord("C"), ord("G"), 3, 3)])),
    ("d == 0 does not seed", fa(R, R, R, V9, V9, V9, X9), 1, LINEAR, dict(max_haplotypes=3),
     dict(sizes=[4, 3], members=[0, 0, 0, 1, 1, 1, 0], haps=[R, V9], sites=[(9, ord("C"), ord("G"), 3, 3)])),
    ("indel without the flag", fa(R, R, R, D9, D9, D9), 1, LINEAR, {}, dict(sizes=[6], members=[0] * 6, sites=[])),
    ("indel with the flag", fa(R, R, R, D9, D9, D9), 1, LINEAR, dict(indels=True),
     dict(sizes=[3, 3], members=[0, 0, 0, 1, 1, 1], haps=[R, D9], sites=[(9, ord("G"), ord("-"), 3, 3)])),
    # two members end before the site: they vote 0 and stay with haplotype 0
    ("member short of the site, semi-global", fa(R, R, R, V9, V9, V9, R[:7], R[:7]), 2, LINEAR, {},
     dict(sizes=[5, 3], members=[0, 0, 0, 1, 1, 1, 0, 0])),
    ("member short of the site, local", fa(R, R, R, V9, V9, V9, R[:7], R[:7]), 0, LINEAR, {},
     dict(sizes=[5, 3], members=[0, 0, 0, 1, 1, 1, 0, 0])),
    ("three haplotypes, max 1", fa(H1, H1, H1, H2, H2, H2, H3, H3, H3), 1, LINEAR, dict(max_haplotypes=1), dict(sizes=[9], members=[0] * 9)),
    # the third haplotype agrees -1 with either profile: the tie goes to k = 0
    ("three haplotypes, max 2", fa(H1, H1, H1, H2, H2, H2, H3, H3, H3), 1, LINEAR, dict(max_haplotypes=2),
     dict(sizes=[6, 3], members=[0, 0, 0, 1, 1, 1, 0, 0, 0])),
    ("three haplotypes, max 3", fa(H1, H1, H1, H2, H2, H2, H3, H3, H3), 1, LINEAR, dict(max_haplotypes=3),
     dict(sizes=[3, 3, 3], members=[0, 0, 0, 1, 1, 1, 2, 2, 2], haps=[H1, H2, H3],
          sites=[(4, ord("T"), ord("A"), 6, 3), (9, ord("G"), ord("C"), 6, 3), (15, ord("G"), ord("T"), 6, 3)])),
    # the lone read with every minor allele seeds a fourth cluster, which is dissolved; it agrees -1 with every profile: k = 0
    ("small cluster dissolved", fa(H1, H1, H1, H2, H2, H2, H3, H3, HX), 1, LINEAR, dict(max_haplotypes=4),
     dict(sizes=[4, 3, 2], members=[0, 0, 0, 1, 1, 1, 2, 2, 0], haps=[H1, H2, H3])),
    # four clusters of two with min_reads 3: none survives
    ("every cluster below min_reads", fa(QA, QA, QB, QB, QC, QC, QD, QD), 1, LINEAR, dict(max_haplotypes=4, min_reads=3),
     dict(sizes=[8], members=[0] * 8)),
    # PY ties between the seeds' profiles and goes to k = 0; the recomputed profile of k = 0 turns at the fourth site and PY moves
    ("a round changes an assignment", fa(P0, PA, PA, PA, PB, PB, PB, PY), 1, LINEAR, {}, dict(members=[0, 0, 0, 0, 1, 1, 1, 1])),
    # within haplotype 0 two low-quality reads say G at base 15 and one high-quality read says T
    ("qualities decide the branch", [(R, QLOW), (R, QLOW), (sub(R, 15, ord("T")), QHIGH), (V9, QLOW), (V9, QLOW), (V9, QLOW)], 1, LINEAR, {},
     dict(sizes=[3, 3], members=[0, 0, 0, 1, 1, 1], haps=[sub(R, 15, ord("T")), V9])),
    ("an empty member", fa(R, R, b"", R, V9, V9, V9), 1, LINEAR, {},
     dict(sizes=[3, 3], members=[0, 0, 0xFF, 0, 1, 1, 1], haps=[R, V9])),
    ("only empty members", fa(b"", b""), 1, LINEAR, {}, dict(sizes=[0], members=[0xFF, 0xFF], haps=[b""], sites=[])),
    ("no member", [], 1, LINEAR, {}, dict(sizes=[0], members=[], haps=[b""], sites=[])),
    ("affine gaps", fa(R, R, R, D9, D9, D9), 1, AFFINE, dict(indels=True),
     dict(sizes=[3, 3], members=[0, 0, 0, 1, 1, 1], haps=[R, D9], sites=[(9, ord("G"), ord("-"), 3, 3)])),
]
