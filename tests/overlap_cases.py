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
