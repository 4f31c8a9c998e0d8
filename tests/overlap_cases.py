"""Hand-built cases for the overlapper (vc_overlap, vc_overlap_sketch), one per edge of the rule in include/vechat_hip.h --
in the manner of fwd_cases.py and trace_cases.py.  tests/test_overlap.py runs the CPU restatement over them (and checks the
answers written out here by hand); tests/test_overlap_gpu.py runs the device over them and compares with the restatement.

Two kinds of sequences:
  * random bases from a fixed seed, for the sketch and for whole-read overlaps;
  * MARKER sequences for the seed and chain edges: 'N' everywhere except for distinct 15-mers ("markers") whose last base sits
    at a chosen position.  With k = 15 and w = 1 every stretch of exactly 15 bases between Ns is one k-mer and one minimizer, so
    the anchors of a pair are exactly the (t_pos, q_pos) of the markers both carry -- each chain problem is written down, not found.
    A marker starts with A and ends with C, so no marker is another's reverse complement: marker anchors are all strand 0.
"""
import numpy as np

K = 15
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def rand(n, seed):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), n))


def marker(i):
    body = "".join("ACGT"[(i >> (2 * d)) & 3] for d in range(13))
    return ("A" + body + "C").encode()


def marked(length, at):
    """'N' * length with marker m ending at position p for every (p, m) of `at`"""
    s = bytearray(b"N" * length)
    for p, m in at:
        assert p - K + 1 >= 0 and p < length and all(c == 78 for c in s[max(p - K, 0):min(p + 2, length)]), (p, m)
        s[p - K + 1:p + 1] = marker(m)
    return bytes(s)


def pair(points, base, t_len=None, q_len=None):
    """a (target, query) pair whose shared markers sit at the given (t_pos, q_pos); marker ids from `base`"""
    t_len = t_len or max(p for p, _ in points) + 1
    q_len = q_len or max(q for _, q in points) + 1
    return (marked(t_len, [(p, base + i) for i, (p, _) in enumerate(points)]),
            marked(q_len, [(q, base + i) for i, (_, q) in enumerate(points)]))


# ---------------------------------------------------------------------------------------------------- sketch
# name -> (sequences, k, w, hand answer or None): the hand answer is the list of (seq, pos) of the table
SKETCH_CASES = {}


def _sk(name, seqs, k=15, w=5, expect=None):
    SKETCH_CASES[name] = (seqs, k, w, expect)


_sk("len_k_minus_1", [rand(14, 1)], expect=[])
_sk("len_k", [rand(15, 2)], expect=[])                                   # one k-mer, no window of 5
_sk("len_k_plus_w_minus_2", [rand(18, 3)], expect=[])                    # four k-mers
_sk("n_in_the_middle", [rand(40, 5) + b"N" + rand(40, 6)])
_sk("n_every_k_bases", [b"".join(rand(14, 10 + i) + b"N" for i in range(8))], expect=[])
_sk("self_reverse_complement_kmer", [rand(20, 7) + b"GAATTC" + rand(20, 8), b"GAATTCGAATTC"], k=6, w=3)
_sk("homopolymer", [b"A" * 50], expect=[(0, p) for p in range(14, 46)])  # equal hashes: the leftmost of every window
_sk("dinucleotide_repeat", [b"AC" * 30])
_sk("lower_case_and_other_bytes", [rand(60, 9).lower() + b"-" + rand(30, 12) + b"R" + rand(25, 13)])
_sk("one_short_of_a_block", [rand(255, 20)])
_sk("exactly_a_block", [rand(256, 21)])
_sk("one_past_a_block", [rand(257, 22)])
_sk("three_blocks", [rand(700, 23)])
_sk("minimizer_window_across_the_block_edge", [rand(250, 24) + b"A" * 30 + rand(100, 25)])
_sk("set_with_empty_sequences", [b"", rand(100, 26), b"", rand(19, 27), b""])
_sk("widest_window_and_longest_kmer", [rand(400, 28)], k=28, w=64)
_sk("w_1_every_kmer", [rand(60, 29)], k=4, w=1)
# len k + w - 1: exactly one window, exactly one minimizer (where, the hash decides)
_sk("len_k_plus_w_minus_1", [rand(19, 4)])

# --------------------------------------------------------------------------------------------------- overlaps
# name -> dict(targets, queries (None: same_set), params, budget_mb (None: default), min_pieces, expect (None, or the list of
# (q_id, t_id, strand, q_begin, q_end, t_begin, t_end, n_anchors, score, matches, block) written out by hand))
OVERLAP_CASES = {}
CHAIN = dict(k=15, w=1, min_overlap=1, drop_internal=0, min_anchors=1, min_chain_score=15)


def _ov(name, targets, queries, params=None, budget_mb=None, min_pieces=1, expect=None):
    OVERLAP_CASES[name] = dict(targets=targets, queries=queries, params=params or {}, budget_mb=budget_mb, min_pieces=min_pieces, expect=expect)


def _line(n, step=20, t0=100, q0=100):
    return [(t0 + step * i, q0 + step * i) for i in range(n)]


# ---- seeds
# marker 1: 2 + 2 entries = max_occ, kept; marker 2: 3 + 2 = max_occ + 1, dropped.  What is left: key (0, 0): markers 1 (two target
# positions x two query positions) -- 4 anchors
_ov("bucket_of_max_occ_and_one_more",
    [marked(400, [(50, 1), (150, 1), (250, 2), (300, 2), (350, 2)])], [marked(400, [(60, 1), (160, 1), (260, 2), (360, 2)])],
    dict(CHAIN, max_occ=4),
    expect=[(0, 0, 0, 46, 161, 36, 151, 2, 30, 30, 115)])
_ov("bucket_of_one_sequence_only", [marked(300, [(50, 3), (120, 3), (200, 3)]), marked(100, [(50, 4)])], None, dict(CHAIN), expect=[])
_ov("identical_sequences_same_set", [rand(600, 40), rand(600, 40)], None, dict(min_overlap=500))
_ov("identical_sequences_two_sets", [rand(600, 40), rand(600, 40)], [rand(600, 40), rand(600, 40)], dict(min_overlap=500))     # (i, i) is a pair here



def unmix(h, k):
    """the k-mer code whose hash (the mix of include/vechat_hip.h on 2k bits) is h: every step of the mix undone, last step first"""
    bits = 2 * k
    m = (1 << bits) - 1

    def unshift(y, s):                                        # x ^ (x >> s) = y
        x = y
        for _ in range(bits // s + 1):
            x = y ^ (x >> s)
        return x

    x = (h * pow(1 + (1 << 31), -1, 1 << bits)) & m
    x = unshift(x, 28)
    x = (x * pow(21, -1, 1 << bits)) & m
    x = unshift(x, 14)
    x = (x * pow(265, -1, 1 << bits)) & m
    x = unshift(x, 24)
    return ((x + 1) * pow((1 << 21) - 1, -1, 1 << bits)) & m  # ~x + (x << 21) = x * (2^21 - 1) - 1


def kmer_of_hash(h, k):
    """the k bases of unmix(h, k), or None when their reverse complement is the smaller code (the hash would then be another's)"""
    x = unmix(h, k)
    s = bytes(b"ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))
    fw, rv = x, sum((3 - ((x >> (2 * i)) & 3)) << (2 * (k - 1 - i)) for i in range(k))
    return s if fw < rv else None


def twins(k, bit, seed):
    """two k-mers whose hashes differ in the one bit `bit` (>= 32) and in no other, and the hashes"""
    rng = np.random.default_rng(seed)
    while True:
        h = int(rng.integers(0, 1 << (2 * k)))
        a, b = kmer_of_hash(h, k), kmer_of_hash(h ^ (1 << bit), k)
        if a and b:
            return a, b, h, h ^ (1 << bit)


# k = 19: two different 19-mers whose 38-bit hashes are equal in their low 32 bits (they differ in bit 32 for the first pair of reads, in bit
# 37 for the second) seed nothing; the 19-mer both reads carry seeds the only anchor.  The tables hold nothing else, so each pair of twins
# is next to each other in every order by hash
_tw = [twins(19, 32, 70), twins(19, 37, 71)]
_sh = [rand(19, 72), rand(19, 73)]
_ov("hashes_equal_in_their_low_32_bits",
    [b"N" * 30 + a + b"N" * 30 + s + b"N" * 10 for (a, _, _, _), s in zip(_tw, _sh)], [b"N" * 30 + b + b"N" * 30 + s + b"N" * 10 for (_, b, _, _), s in zip(_tw, _sh)],
    dict(CHAIN, k=19, min_chain_score=19),
    expect=[(0, 0, 0, 79, 98, 79, 98, 1, 19, 19, 19), (1, 1, 0, 79, 98, 79, 98, 1, 19, 19, 19)])

# ---- chains: keys of 1, 2, 3, 64, 65 and 130 colinear anchors, 20 apart: score 15 n, every anchor in the chain
_sizes = (1, 2, 3, 64, 65, 130)
_pairs = [pair(_line(n), 1000 * (i + 1)) for i, n in enumerate(_sizes)]
_ov("keys_of_1_2_3_64_65_130_anchors", [t for t, _ in _pairs], [q for _, q in _pairs], dict(CHAIN),
    expect=[(i, i, 0, 86, 101 + 20 * (n - 1), 86, 101 + 20 * (n - 1), n, 15 * n, 15 * n, 15 + 20 * (n - 1)) for i, n in enumerate(_sizes)])


def _lookback(decoys, base):
    """A = (100, 100) and F on its diagonal with `decoys` anchors between them in the order, each admissible with nothing (their
    q positions fall while t rises, far off the diagonal): F sees A only if A is among the 64 anchors in front of it"""
    pts = [(100, 100)] + [(100 + 16 * (i + 1), 40000 - 16 * i) for i in range(decoys)] + [(100 + 16 * (decoys + 1), 100 + 16 * (decoys + 1))]
    return pair(pts, base)


_a, _b = _lookback(63, 20000), _lookback(64, 21000)
_ov("predecessor_64_back_and_65_back", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN),
    expect=[(0, 0, 0, 86, 1125, 86, 1125, 2, 30, 30, 1039),          # A -> F, 64 back
            (1, 1, 0, 86, 101, 86, 101, 1, 15, 15, 15)])               # 65 back: every anchor alone, the first one wins the tie
_a, _b = pair([(100, 100), (300, 300)], 30000), pair([(100, 100), (301, 301)], 30010)
_ov("dt_of_max_gap_and_one_more", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN, max_gap=200),
    expect=[(0, 0, 0, 86, 301, 86, 301, 2, 30, 30, 215), (1, 1, 0, 86, 101, 86, 101, 1, 15, 15, 15)])
# dt = 190 / 191 is within the limit both times; dq = 200 is, 201 is not.  d = 10: cost = 10 * 15 / 100 + ilog2(10) / 2 = 1 + 1, f = 28
_a, _b = pair([(100, 100), (290, 300)], 30400), pair([(100, 100), (291, 301)], 30410)
_ov("dq_of_max_gap_and_one_more", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN, max_gap=200),
    expect=[(0, 0, 0, 86, 301, 86, 291, 2, 28, 30, 215), (1, 1, 0, 86, 101, 86, 101, 1, 15, 15, 15)])
# marker X twice on the query: anchors (100, 100), (100, 160), (120, 180).  The first two share t_pos (dt = 0: no link); Y follows both,
# from (100, 100) with d = 60 (cost 9 + 2, f = 19), from (100, 160) with d = 0 (f = 30)
_ov("two_anchors_on_one_target_position", [marked(200, [(100, 30420), (120, 30421)])], [marked(260, [(100, 30420), (160, 30420), (180, 30421)])],
    dict(CHAIN), expect=[(0, 0, 0, 146, 181, 86, 121, 2, 30, 30, 35)])
# a reverse strand with the coordinates written out: the query is the reverse complement of a three-marker line, once as long as the
# line (its markers end up at 0..55) and once with 59 bases in front of that (59..114); on the target they stay at 86..141
_a = pair(_line(3), 30430)
_ov("reverse_strand_chain_by_hand", [_a[0]], [rc(_a[1]), b"N" * 59 + rc(_a[1])], dict(CHAIN),
    expect=[(0, 0, 1, 0, 55, 86, 141, 3, 45, 45, 55), (1, 0, 1, 59, 114, 86, 141, 3, 45, 45, 55)])
# six 15-mers one base apart (k is odd: none is its own reverse complement): every link has dt = dq = 1 and gains 1, not k
_s = b"ACGGTCATTGCAAGCTTACG"
_ov("adjacent_kmers_gain_below_k", [b"N" * 100 + _s + b"N" * 80], [b"N" * 50 + _s + b"N" * 30], dict(CHAIN),
    expect=[(0, 0, 0, 50, 70, 100, 120, 6, 20, 20, 20)])
# positions that need 17 bits: 274 and 259 sketch blocks, nearly all of them without a k-mer
_a = pair([(70000 + 20 * i, 66000 + 20 * i) for i in range(5)], 30440, t_len=70200, q_len=66200)
_ov("positions_beyond_16_bits", [_a[0]], [_a[1]], dict(CHAIN), expect=[(0, 0, 0, 65986, 66081, 69986, 70081, 5, 75, 75, 95)])
# d = 50: cost = 50 * 15 / 100 + ilog2(50) / 2 = 7 + 2 = 9, f = 15 + 15 - 9 = 21;  d = 51: not admissible
_a, _b = pair([(100, 100), (200, 250)], 30020), pair([(100, 100), (200, 251)], 30030)
_ov("diagonal_shift_of_bandwidth_and_one_more", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN, bandwidth=50),
    expect=[(0, 0, 0, 86, 251, 86, 201, 2, 21, 30, 165), (1, 1, 0, 86, 101, 86, 101, 1, 15, 15, 15)])
# P1 = (100, 120) and P2 = (120, 100) cannot follow each other; F = (300, 300) gets 15 + 15 - (20 * 15 / 100 + 4 / 2) = 25 from both: P2, the later one
_a = pair([(100, 120), (120, 100), (300, 300)], 30040)
_ov("two_predecessors_of_equal_value", [_a[0]], [_a[1]], dict(CHAIN), expect=[(0, 0, 0, 86, 301, 106, 301, 2, 25, 30, 215)])
# two runs 2000 off each other's diagonal: equal scores -> the earlier end; a fourth anchor on the second -> the second
_r1, _r2 = _line(3), _line(3, t0=3000, q0=1000)
_a, _b = pair(_r1 + _r2, 30050), pair(_r1 + _line(4, t0=3000, q0=1000), 30060)
_ov("two_runs_on_two_diagonals", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN),
    expect=[(0, 0, 0, 86, 141, 86, 141, 3, 45, 45, 55), (1, 1, 0, 986, 1061, 2986, 3061, 4, 60, 60, 75)])
# 45 = min_chain_score is kept; one link with d = 4 costs 0 + ilog2(4) / 2 = 1: 44 is not
_a, _b = pair(_line(3), 30070), pair([(100, 100), (120, 120), (140, 144)], 30080)
_ov("score_of_min_chain_score_and_one_less", [_a[0], _b[0]], [_a[1], _b[1]], dict(CHAIN, min_chain_score=45),
    expect=[(0, 0, 0, 86, 141, 86, 141, 3, 45, 45, 55)])
_ov("min_anchors", [_a[0], pair(_line(2), 30090)[0]], [_a[1], pair(_line(2), 30090)[1]], dict(CHAIN, min_anchors=3),
    expect=[(0, 0, 0, 86, 141, 86, 141, 3, 45, 45, 55)])

# ---- records
_t = rand(1500, 50)
_ov("reverse_strand_touching_both_query_ends", [_t], [rc(_t[200:1000])], {})
_ov("containment_is_kept", [_t], [_t[300:1100]], {})
_ov("internal_match_is_dropped", [_t], [rand(1200, 51) + _t[300:1100] + rand(1200, 52)], {}, expect=[])
# one pair, two keys: the first half matches forward, the second reversed -- a record for each strand (no hand answer: random bases)
_x, _y = rand(600, 90), rand(600, 91)
_ov("both_strands_of_one_pair", [_x + _y], [_x + rc(_y)], dict(drop_internal=0))
# block = 485 + 15 = 500 is kept, 499 is not (defaults: min_overlap 500)
_a, _b = pair([(100, 100), (585, 585)], 30100), pair([(100, 100), (584, 584)], 30110)
_ov("block_of_500_and_499", [_a[0], _b[0]], [_a[1], _b[1]], dict(k=15, w=1, min_anchors=2, min_chain_score=30, drop_internal=0),
    expect=[(0, 0, 0, 86, 586, 86, 586, 2, 30, 30, 500)])
# 21 anchors 200 apart: block 4015, slack 3 * 4015 / 21 = 573.  Left end 1573 / 1574 on both reads, right 0: the overhang after the slack is
# 1000 / 1001, and 5 * (4015 + 573) >= 4 * (4015 + 573 + 1000) holds, so only "overhang > 1000" decides
_a = pair(_line(21, step=200, t0=1587, q0=1587), 30200)
_b = pair(_line(21, step=200, t0=1588, q0=1588), 30300)
_ov("overhang_at_the_limit_and_one_past", [_a[0], _b[0]], [_a[1], _b[1]], dict(k=15, w=1),
    expect=[(0, 0, 0, 0, 5588, 0, 5588, 21, 315, 315, 5588)])              # kept, and then taken out to the read ends
# a dense chain, 401 anchors 16 apart: block 6415, slack 3 * 6415 / 401 = 47: left end 1047 is kept, 1048 is not
_a = pair(_line(401, step=16, t0=1061, q0=1061), 31000)
_b = pair(_line(401, step=16, t0=1062, q0=1062), 32000)
_ov("overhang_limit_with_a_dense_chain", [_a[0], _b[0]], [_a[1], _b[1]], dict(k=15, w=1),
    expect=[(0, 0, 0, 0, 7462, 0, 7462, 401, 6015, 6015, 7462)])

# ---- budget: six overlapping reads of one genome; under a budget of one anchor every target is a piece of its own
_g = rand(4000, 60)
_reads = [_g[s:s + 1500] if i % 2 == 0 else rc(_g[s:s + 1500]) for i, s in enumerate((0, 400, 800, 1200, 1600, 2500))]
_ov("default_budget", _reads, None, {})
_ov("three_or_more_target_pieces", _reads, None, {}, budget_mb=0.0001, min_pieces=3)
_ov("pieces_with_two_sets", _reads[:4], _reads[2:], {}, budget_mb=0.0001, min_pieces=3)


# ---------------------------------------------------------------------------------------------------- repeats
def repeat_reads():
    """four reads across a genome with a 37-base unit repeated 30 times in the middle, one reverse-complemented: every minimizer of
    the unit fills a bucket of ~100 entries, and the keys between two reads hold thousands of anchors, nearly all off the diagonal"""
    g = rand(800, 78) + rand(37, 77) * 30 + rand(800, 79)
    return [g[0:1500], g[400:2000], rc(g[700:2400]), g[1000:]]


# ------------------------------------------------------------------------------------------------------ sweep
SWEEP_SEED = 20261028          # chosen so that 21 of the 24 configurations give records, 221 together (tests/test_overlap.py asserts >= 16 and >= 200)
SWEEP_CONFIGS = 24


def sweep(seed=SWEEP_SEED, n=SWEEP_CONFIGS):
    """n random configurations from one seed, each dict(targets, queries (None: same_set), params, budget_mb): every parameter of
    the rule drawn from a few values on both sides of what matters, 6 to 10 reads of 0 to 900 bases cut from a 2.5 kb genome that
    holds a 30-base unit 8 times -- some reverse-complemented, some lower-cased, some with a foreign byte spliced in, one empty
    and one shorter than k."""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(4, 28)
        params = dict(k=k, w=rng.choice([1, 3, 5, 10, 64]), max_occ=rng.choice([2, 10, 100]), max_gap=rng.choice([50, 500, 5000]),
                      bandwidth=rng.choice([5, 50, 500]), min_anchors=rng.choice([1, 3]), min_chain_score=rng.choice([k, 40]),
                      min_overlap=rng.choice([1, 200, 500]), drop_internal=rng.choice([0, 1]))
        two_sets = rng.choice([False, True])
        budget_mb = rng.choice([None, 0.01])
        g = bytearray(rand(2500, rng.randrange(1 << 30)))
        at = rng.randrange(0, 2500 - 240)
        g[at:at + 240] = rand(30, rng.randrange(1 << 30)) * 8
        g = bytes(g)
        reads = []
        for _ in range(rng.randint(6, 10)):
            ln = rng.randint(600, 900) if rng.random() < 0.7 else rng.randint(0, 900)      # mostly long enough to overlap a neighbour
            s = rng.randint(0, 2500 - ln)
            r = g[s:s + ln]
            if rng.random() < 0.4:
                r = rc(r)
            if rng.random() < 0.25:
                r = r.lower()
            if ln and rng.random() < 0.3:
                p = rng.randrange(ln)
                r = r[:p] + bytes([rng.choice(b"NnR-*\x00\xc1")]) + r[p:]
            reads.append(r)
        a, b = rng.sample(range(len(reads)), 2)
        reads[a] = b""
        s = rng.randint(0, 2400)
        reads[b] = g[s:s + rng.randint(1, k - 1)]
        if two_sets:                                          # two reads are in both sets
            cut = len(reads) // 2
            targets, queries = reads[:cut + 1], reads[cut - 1:]
        else:
            targets, queries = reads, None
        out.append(dict(targets=targets, queries=queries, params=params, budget_mb=budget_mb))
    return out
