"""Hand-built cases for the demultiplexer (vc_demux; the rule is in include/vechat_hip.h): a few reads of at most a few hundred bases
each.  CASES[name] = dict(reads, quals or None, patterns, labels or None, sides or None, params, expect), where expect maps a field
of vc_demux_out to the whole list written out by hand, or to {index: value} where only some entries are; a case without a
hand-written answer still pins the device to the restatement.  tests/test_demux.py runs tests/demux_ref.py on the table,
tests/test_demux_gpu.py the device."""
import numpy as np

import demux_ref as R

U = R.UNASSIGNED
COMP = bytes.maketrans(b"ACGT", b"TGCA")
rc = lambda s: bytes(s).translate(COMP)[::-1]
B1 = b"ACGTTGCAAGCTAGGATCCTAGTC"                      # two barcodes of 24 bases, far from each other and from any homopolymer
B2 = b"GATCGGTACCATGCAAGTCCGTTA"
BX, BY = B1[:10] + b"A" + B1[11:], B1[:10] + b"T" + B1[11:]          # B1 (a G there) with one substitution each: both at distance 1 of B1
P64 = b"ACGTTGCAAGCTAGGATCCTAGTCGATCGGTACCATGCAAGTCCGTTAACTGGACTTCAGGCATA"[:64]
PRIMER = b"GGACTACNVGGGTWTCTAAT"                      # three degenerate positions
T60 = b"T" * 60
CASES = {}


def case(name, reads, patterns, labels=None, sides=None, quals=None, expect=None, **params):
    assert name not in CASES
    CASES[name] = dict(reads=[bytes(r) for r in reads], quals=quals, patterns=[bytes(p) for p in patterns], labels=labels, sides=sides,
                       params=params, expect=expect or {})


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


# ------------------------------------------------------------------------------------------------ the classes, step by step
both = B1 + T60 + rc(B1)
case("both_ends_exact", [both], [B1, B2],
     expect=dict(v_pat=[0, 0], v_dist=[0, 0], v_start=[0, 0], v_end=[24, 24], v_second=[255, 255], klass=[R.BOTH_ENDS], label=[0], flip=[0], begin=[24], end=[84],
                 piece_off=[0, 60], grp_off=[0, 1, 1], grp_reads=[0]))
case("trim_0_keeps_everything", [both], [B1, B2], trim=0, expect=dict(klass=[R.BOTH_ENDS], begin=[0], end=[108]))
case("trim_2_keeps_the_pattern", [B"GG" + both + b"G"], [B1, B2], trim=2, expect=dict(v_start=[2, 1], v_end=[26, 25], begin=[2], end=[110]))
case("every_class", [T60, B1 + T60, T60 + rc(B2), B1 + T60 + rc(B2), both], [B1, B2],
     expect=dict(klass=[R.NONE, R.ONE_END, R.ONE_END, R.CONFLICT, R.BOTH_ENDS], label=[U, 0, 1, U, 0], begin=[0, 24, 0, 24, 24], end=[60, 84, 60, 84, 84],
                 grp_off=[0, 2, 3], grp_reads=[1, 4, 2]))
case("every_class_require_both", [T60, B1 + T60, T60 + rc(B2), B1 + T60 + rc(B2), both], [B1, B2], flags=R.REQUIRE_BOTH,
     expect=dict(klass=[R.NONE, R.ONE_END, R.ONE_END, R.CONFLICT, R.BOTH_ENDS], label=[U, U, U, U, 0], grp_off=[0, 1, 1], grp_reads=[4]))
# BX and BY of labels 0 and 1 are both one error from B1: an end with B1 is ambiguous at the default margin
case("ambiguous_with_none_label_and_ambiguous", [B1 + T60, B1 + T60 + rc(B2), both, B2 + T60 + rc(B2)], [BX, BY, B2], labels=[0, 1, 2],
     expect=dict(v_pat={0: 0, 2: 0, 3: 2}, v_dist={0: 1, 3: 0}, v_second={0: 1, 3: 255}, klass=[R.AMBIGUOUS, R.AMBIGUOUS, R.AMBIGUOUS, R.BOTH_ENDS], label=[U, U, U, 2],
                 begin=[24, 24, 24, 24], grp_off=[0, 0, 0, 1]))
for margin, klass, label in ((0, R.ONE_END, 0), (1, R.AMBIGUOUS, U), (2, R.AMBIGUOUS, U)):
    case(f"equal_d_two_labels_margin_{margin}", [B1 + T60], [BX, BY], labels=[0, 1], min_margin=margin,
         expect=dict(v_pat=[0, U], v_dist=[1, 255], v_second=[1, 255], klass=[klass], label=[label]))
case("equal_d_one_label_is_not_ambiguous_and_labels_without_reads", [B1 + T60], [BX, BY], labels=[5, 5],
     expect=dict(v_pat=[0, U], v_second=[255, 255], klass=[R.ONE_END], label=[5], grp_off=[0, 0, 0, 0, 0, 0, 1], grp_reads=[0]))
case("one_error_apart_is_ambiguous_at_margin_2_only", [B1 + T60, B1 + T60], [B1, BX], labels=[0, 1],
     expect=dict(v_dist={0: 0}, v_second={0: 1}, klass=[R.AMBIGUOUS, R.AMBIGUOUS]))
case("one_error_apart_margin_1", [B1 + T60], [B1, BX], labels=[0, 1], min_margin=1, expect=dict(klass=[R.ONE_END], label=[0], v_second=[1, 255]))

# ---------------------------------------------------------------------------------- strands: a forward and a reverse primer
plus_read = B1 + b"AAACCC" + T60 + rc(B2)
SIDED = dict(patterns=[B1, B2], labels=[0, 0], sides=[R.HEAD, R.TAIL])
case("plus_and_minus_evidence", [plus_read, rc(plus_read), B1 + T60, B2 + T60, T60 + rc(B2), T60 + rc(B1), B1 + T60 + rc(B1)], **SIDED,
     expect=dict(klass=[R.BOTH_ENDS, R.BOTH_ENDS, R.ONE_END, R.ONE_END, R.ONE_END, R.ONE_END, R.CONFLICT], flip=[0, 1, 0, 1, 0, 1, 0], label=[0, 0, 0, 0, 0, 0, U],
                 v_pat=[0, 1, 1, 0, 0, U, 1, U, U, 1, U, 0, 0, 0]))
minus = B2 + b"AAACCC" + rc(B1)
case("flip_with_qualities", [minus, B1 + b"AAACCC" + rc(B2)], quals=[bytes(range(40, 40 + len(minus))), bytes(range(40, 40 + len(minus)))], flags=R.ORIENT, **SIDED,
     expect=dict(flip=[1, 0], begin=[24, 24], end=[30, 30], pc_bases=b"GGGTTT" + b"AAACCC", pc_quals=bytes(range(40 + 24, 40 + 30))[::-1] + bytes(range(40 + 24, 40 + 30))))
case("flip_is_reported_but_not_applied_without_orient", [minus], quals=[bytes(range(40, 40 + len(minus)))], **SIDED,
     expect=dict(flip=[1], pc_bases=b"AAACCC", pc_quals=bytes(range(64, 70))))

# ---------------------------------------------------------------------------------------------- lengths, windows, the ends
for m in (1, 31, 32, 33, 63, 64):
    case(f"pattern_length_{m}", [b"GGG" + P64[:m] + b"G" * 20, b"GGG" + P64[:m]], [P64[:m]], max_err_permille=0,
         expect=dict(v_pat=[0, U, 0, U], v_dist=[0, 255, 0, 255], v_start=[3, 0, 3, 0], v_end=[3 + m, 0, 3 + m, 0], begin=[3 + m, 3 + m], end=[23 + m, 3 + m]))
# a substitution at pattern position 31 and a deletion of position 32; and the same two around 30 / 33
case("errors_straddle_positions_31_and_32", [b"TT" + P64[:31] + b"T" + P64[33:] + T60, b"TT" + P64[:30] + b"A" + P64[31:33] + P64[34:] + T60], [P64],
     expect=dict(v_dist={0: 2, 2: 2}, v_start={0: 2, 2: 2}, v_end={0: 65, 2: 65}))
case("view_shorter_than_the_pattern", [B1[:10]], [B1], max_err_permille=1000, expect=dict(v_pat={0: 0}, v_dist={0: 14}, v_start={0: 0}, v_end={0: 10}))
case("length_0_and_1", [b"", b"A", b"C"], [b"A", B1],
     expect=dict(v_pat=[U, U, 0, U, U, U], klass=[R.NONE, R.ONE_END, R.NONE], label=[U, 0, U], begin=[0, 1, 0], end=[0, 1, 1], piece_off=[0, 0, 0, 1], pc_bases=b"C"))
case("window_1", [b"ACCT", b"CCCA"], [b"A"], window=1,
     expect=dict(v_pat=[0, 0, U, U], v_end=[1, 1, 0, 0], klass=[R.BOTH_ENDS, R.NONE], begin=[1, 0], end=[3, 4], pc_bases=b"CC" + b"CCCA"))
case("overlapping_hits_give_an_empty_piece", [b"TTACGTACGTTT"], [b"ACGTACGT"], window=10, max_err_permille=0,
     expect=dict(v_start=[2, 2], v_end=[10, 10], klass=[R.BOTH_ENDS], begin=[10], end=[10], piece_off=[0, 0]))
case("read_shorter_than_the_window", [B1 + b"GG" + rc(B1)], [B1], expect=dict(v_end=[24, 24], begin=[24], end=[26], pc_bases=b"GG"))
case("smaller_end_wins_at_equal_distance", [b"ACGTTTACGT" + T60], [b"ACGT"], max_err_permille=0, expect=dict(v_start={0: 0}, v_end={0: 4}))
# CAAGT against ..CAAAGT: one error whether the hit starts at 2 (an insertion), 3 (a substitution) or 4 (a deletion): the shortest
case("shortest_hit_differs_from_the_longest", [b"TTCAAAGT" + T60], [b"CAAGT"], expect=dict(v_dist={0: 1}, v_start={0: 4}, v_end={0: 8}, begin=[8]))
case("max_err_1000_accepts_everything", [T60, b"G"], [B1, b"ACGT"], labels=[0, 0], max_err_permille=1000, expect=dict(klass=[R.BOTH_ENDS, R.BOTH_ENDS]))

# ------------------------------------------------------------------------------------------------------------------ codes
case("iupac_n_and_r", [b"ACGT" + T60, b"AAAT" + T60, b"ACCT" + T60], [b"ANRT"], max_err_permille=0, window=10,
     expect=dict(v_pat={0: 0, 2: 0, 4: U}, klass={0: R.ONE_END, 1: R.ONE_END}))
case("primer_with_three_degenerate_positions", [b"GGACTACAGGGGTATCTAAT" + T60, b"GGACTACCTGGGTTTCTAAT" + T60, b"GGACTACACGGGTGTCTAAT" + T60], [PRIMER],
     expect=dict(v_dist={0: 0, 2: 1, 4: 1}, v_end={0: 20, 2: 20, 4: 20}))
case("n_and_lower_case_in_a_read_match_nothing", [b"ACNT" + T60, b"ACgT" + T60, b"ANGT" + T60, b"ACGT" + T60], [b"ACGT", b"ANGT"], labels=[0, 0], max_err_permille=250,
     expect=dict(v_dist={0: 1, 2: 1, 4: 1, 6: 0}, v_pat={0: 0, 2: 0, 4: 0, 6: 0}))
case("lower_case_is_its_own_complement", [b"acgtACGTTTTT"], [b"AAAAACGT"], sides=[R.HEAD], flags=R.ORIENT, max_err_permille=0,
     expect=dict(v_pat=[U, 0], flip=[1], begin=[0], end=[4], pc_bases=b"acgt"[::-1]))


# --------------------------------------------------------------------------------------------- pattern counts, block edges
def many_patterns(P, seed):
    """P seeded patterns of lengths 1..64 over a few labels and 9 reads that carry some of them, with errors: 18 P triples -- from
    P = 15 on more than one block of 256, and with a small budget more than one piece"""
    rng = np.random.default_rng(seed)
    patterns = [random_bases(rng, int(rng.integers(1, 65))) for _ in range(P)]
    reads = []
    for i in range(9):
        a, b = patterns[int(rng.integers(P))], patterns[int(rng.integers(P))]
        body = bytearray(a + random_bases(rng, int(rng.integers(0, 90))) + rc(b))
        for _ in range(int(rng.integers(0, 5))):
            body[int(rng.integers(len(body)))] = int(rng.choice(np.frombuffer(b"ACGTN", np.uint8)))
        reads.append(bytes(body) if i else b"")
    return reads, patterns, [int(x) for x in rng.integers(0, 7, P)], [int(x) for x in rng.integers(0, 3, P)]


for P in (1, 63, 64, 65):
    reads, patterns, labels, sides = many_patterns(P, 100 + P)
    case(f"patterns_{P}", reads, patterns, labels, sides, flags=R.ALL_HITS | R.ORIENT, window=40)


# ------------------------------------------------------------------------------------------------------------ the sweep
def sweep():
    """200 seeded reads of 0..600 bases in 20 configurations of ten: every P of 1, 7, 64, 65, 130 with every window of 1, 33, 150, 600;
    flags, trim, margin and error rate change from one configuration to the next, qualities come with every other one."""
    rng = np.random.default_rng(11)
    out = []
    for i, (P, window) in enumerate((P, w) for P in (1, 7, 64, 65, 130) for w in (1, 33, 150, 600)):
        patterns = [random_bases(rng, int(rng.integers(1, 65)) if rng.random() < 0.5 else int(rng.integers(1, 25))) for _ in range(P)]
        reads = []
        for k in range(10):
            n = int(rng.integers(0, 601)) if k or i % 5 else 0         # every fifth configuration starts with an empty read
            body = bytearray(random_bases(rng, n))
            for end in (0, 1):                                # most reads carry a pattern near each end, with errors
                if n and rng.random() < 0.8:
                    p = bytearray(patterns[int(rng.integers(P))] if not end else rc(patterns[int(rng.integers(P))]))
                    for _ in range(int(rng.integers(0, 4))):
                        p[int(rng.integers(len(p)))] = int(rng.choice(np.frombuffer(b"ACGTNa", np.uint8)))
                    at = int(rng.integers(0, 12))
                    if end:
                        body[max(n - at - len(p), 0):max(n - at, 0)] = p[-max(n - at, 0):] if n - at < len(p) else p
                    else:
                        body[at:at + len(p)] = p
            reads.append(bytes(body[:max(n, 1)]) if n else b"")
        out.append(dict(reads=reads, quals=[bytes(33 + (k * 7 + j) % 60 for j in range(len(r))) for k, r in enumerate(reads)] if i % 2 else None,
                        patterns=patterns, labels=[int(x) for x in rng.integers(0, max(P // 3, 1), P)], sides=[int(x) for x in rng.integers(0, 3, P)],
                        params=dict(window=window, max_err_permille=(200, 0, 350, 1000)[i % 4], min_margin=(2, 0, 1, 5)[(i // 4) % 4], trim=i % 3,
                                    flags=(i % 8) ^ ((i // 8) % 8) | (R.ALL_HITS if i % 5 == 0 else 0))))
    return out
