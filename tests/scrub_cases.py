"""Hand-built cases of the scrub rule (include/vechat_hip.h, vc_scrub).  A case is a dict: lengths, intervals [(read, begin, end)],
params, and `expect` -- the answer written out by hand as regions [(read, begin, end)], klass, bad_total, pieces [(read, begin,
end)] -- or None where the case is generated and only the restatement (tests/scrub_ref.py) knows the answer.  tests/test_scrub.py
runs the restatement on every case; tests/test_scrub_gpu.py the device, with bases and qualities from reads_of()."""
import numpy as np

CLEAN, BAD_ENDS, CHIMERIC, NOT_COVERED = 0, 1, 2, 3


def case(lengths, intervals, expect=None, **params):
    return dict(lengths=list(lengths), intervals=[tuple(x) for x in intervals], params=params, expect=expect)


def answer(regions, klass, bad_total, pieces):
    return dict(regions=regions, klass=klass, bad_total=bad_total, pieces=pieces)


def reads_of(lengths, seed=1):
    """(bases, qualities) for the lengths of a case: every byte drawn, so a piece copied from the wrong place shows"""
    rng = np.random.default_rng(seed)
    reads = [rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes() for n in lengths]
    quals = [rng.integers(33, 74, n).astype(np.uint8).tobytes() for n in lengths]
    return reads, quals


CASES = {
    # a read nobody overlaps is one region over all of it, and NOT_COVERED at any max_bad_permille below 1000
    "no_interval_between_two_reads_that_have_some": case(
        [10, 8, 10], [(0, 0, 10), (2, 0, 10)],
        answer([(1, 0, 8)], [CLEAN, NOT_COVERED, CLEAN], [0, 8, 0], [(0, 0, 10), (2, 0, 10)])),
    "first_and_last_read_without_intervals": case(
        [5, 6, 7], [(1, 0, 6)],
        answer([(0, 0, 5), (2, 0, 7)], [NOT_COVERED, CLEAN, NOT_COVERED], [5, 0, 7], [(1, 0, 6)])),
    "no_interval_at_all": case(
        [3, 0, 4], [],
        answer([(0, 0, 3), (2, 0, 4)], [NOT_COVERED, CLEAN, NOT_COVERED], [3, 0, 4], [])),
    "length_0_read": case(
        [4, 0, 4], [(0, 0, 4), (2, 1, 3)],
        answer([(2, 0, 1), (2, 3, 4)], [CLEAN, CLEAN, BAD_ENDS], [0, 0, 2], [(0, 0, 4), (2, 1, 3)]), max_bad_permille=1000),
    "length_1_reads": case(
        [1, 1], [(0, 0, 1)],
        answer([(1, 0, 1)], [CLEAN, NOT_COVERED], [0, 1], [(0, 0, 1)])),
    # coverage exactly c and exactly c + 1 side by side
    "coverage_0_beside_1_with_c_0": case(
        [20], [(0, 0, 10)],
        answer([(0, 10, 20)], [BAD_ENDS], [10], [(0, 0, 10)]), max_bad_permille=1000),
    "coverage_2_beside_3_with_c_2": case(
        [20], [(0, 0, 20), (0, 0, 20), (0, 0, 10)],
        answer([(0, 10, 20)], [BAD_ENDS], [10], [(0, 0, 10)]), coverage=2, max_bad_permille=1000),
    "interval_beginning_at_0_and_one_ending_at_len": case(
        [30], [(0, 0, 12), (0, 20, 30)],
        answer([(0, 12, 20)], [CHIMERIC], [8], [(0, 0, 12), (0, 20, 30)])),
    # 700 intervals end and 700 begin at position 50: a run of 1 400 equal keys, events 700 .. 2 099 of 2 800, across five blocks of 256
    "many_intervals_sharing_one_endpoint": case(
        [9, 100, 9], [(0, 0, 9)] + [(1, 10, 50)] * 700 + [(1, 50, 90)] * 700 + [(2, 0, 9)],
        answer([(1, 0, 10), (1, 90, 100)], [CLEAN, BAD_ENDS, CLEAN], [0, 20, 0], [(0, 0, 9), (1, 10, 90), (2, 0, 9)])),
    # ... and with c = 700 the four stretches of coverage 0, 700, 700, 0 are one region
    "many_intervals_sharing_one_endpoint_all_bad": case(
        [100], [(0, 10, 50)] * 700 + [(0, 50, 90)] * 700,
        answer([(0, 0, 100)], [BAD_ENDS], [100], []), coverage=700, max_bad_permille=1000),
    # one interval ends where another begins: the coverage stays 1, nothing may split there
    "begin_and_end_at_the_same_position": case(
        [40], [(0, 5, 20), (0, 20, 35)],
        answer([(0, 0, 5), (0, 35, 40)], [BAD_ENDS], [10], [(0, 5, 35)])),
    "begin_and_end_at_the_same_position_inside_a_region": case(
        [40], [(0, 5, 20), (0, 20, 35)],
        answer([(0, 0, 40)], [BAD_ENDS], [40], []), coverage=1, max_bad_permille=1000),
    # coverage 3 | 1 | 2 | 3 with c = 2: the two bad segments are one region; 1000 * 30 == 600 * 50 exactly
    "adjacent_bad_segments_of_different_coverage": case(
        [50], [(0, 0, 10)] * 3 + [(0, 40, 50)] * 3 + [(0, 10, 25)] + [(0, 25, 40)] * 2,
        answer([(0, 10, 40)], [CHIMERIC], [30], [(0, 0, 10), (0, 40, 50)]), coverage=2, max_bad_permille=600),
    # 600 segments of two bases with coverage 2, 1, 2, 1, ... and c = 2: one region over more than two blocks of segments
    "adjacent_bad_segments_across_block_boundaries": case(
        [7, 1300], [(0, 0, 7)] + [(1, 2 * i, 2 * i + 2) for i in range(600)] + [(1, 4 * i, 4 * i + 2) for i in range(300)] + [(1, 1200, 1300)] * 3,
        answer([(0, 0, 7), (1, 0, 1200)], [BAD_ENDS, BAD_ENDS], [7, 1200], [(1, 1200, 1300)]), coverage=2, max_bad_permille=1000),
    # a region at the left end only, at the right end only, strictly inside, and all three; the last with 1000 * 40 == 400 * 100
    "region_left_right_inside_and_all_three": case(
        [100, 100, 100, 100], [(0, 10, 100), (1, 0, 90), (2, 0, 40), (2, 60, 100), (3, 10, 40), (3, 60, 90)],
        answer([(0, 0, 10), (1, 90, 100), (2, 40, 60), (3, 0, 10), (3, 40, 60), (3, 90, 100)], [BAD_ENDS, BAD_ENDS, CHIMERIC, CHIMERIC],
               [10, 10, 20, 40], [(0, 10, 100), (1, 0, 90), (2, 0, 40), (2, 60, 100), (3, 10, 40), (3, 60, 90)])),
    "region_at_the_left_end_alone": case([100], [(0, 10, 100)], answer([(0, 0, 10)], [BAD_ENDS], [10], [(0, 10, 100)])),
    "region_at_the_right_end_alone": case([100], [(0, 0, 90)], answer([(0, 90, 100)], [BAD_ENDS], [10], [(0, 0, 90)])),
    "region_inside_alone": case([100], [(0, 0, 40), (0, 60, 100)], answer([(0, 40, 60)], [CHIMERIC], [20], [(0, 0, 40), (0, 60, 100)])),
    # 1000 * 400 == 400 * 1000 is not NOT_COVERED; one bad base more is
    "bad_total_exactly_at_the_limit_and_one_more": case(
        [1000, 1000], [(0, 400, 1000), (1, 401, 1000)],
        answer([(0, 0, 400), (1, 0, 401)], [BAD_ENDS, NOT_COVERED], [400, 401], [(0, 400, 1000)])),
    "max_bad_permille_0": case(
        [10, 10], [(0, 0, 10), (1, 0, 9)],
        answer([(1, 9, 10)], [CLEAN, NOT_COVERED], [0, 1], [(0, 0, 10)]), max_bad_permille=0),
    "max_bad_permille_1000": case(
        [10, 10], [(1, 3, 4)],
        answer([(0, 0, 10), (1, 0, 3), (1, 4, 10)], [BAD_ENDS, BAD_ENDS], [10, 9], [(1, 3, 4)]), max_bad_permille=1000),
    "min_piece_drops_a_short_middle_piece": case(
        [100], [(0, 0, 30), (0, 40, 45), (0, 60, 100)],
        answer([(0, 30, 40), (0, 45, 60)], [CHIMERIC], [25], [(0, 0, 30), (0, 60, 100)]), min_piece=10),
    "min_piece_exactly_met": case(
        [100], [(0, 0, 30), (0, 40, 50), (0, 60, 100)],
        answer([(0, 30, 40), (0, 50, 60)], [CHIMERIC], [20], [(0, 0, 30), (0, 40, 50), (0, 60, 100)]), min_piece=10),
    "every_piece_dropped": case(
        [30, 12], [(0, 5, 10), (0, 20, 25), (1, 0, 12)],
        answer([(0, 0, 5), (0, 10, 20), (0, 25, 30)], [CHIMERIC, CLEAN], [20, 0], [(1, 0, 12)]), min_piece=6, max_bad_permille=1000),
    # the output offsets skip a NOT_COVERED read
    "not_covered_read_between_two_kept_ones": case(
        [20, 20, 20], [(0, 0, 20), (2, 0, 20), (1, 0, 5)],
        answer([(1, 5, 20)], [CLEAN, NOT_COVERED, CLEAN], [0, 15, 0], [(0, 0, 20), (2, 0, 20)])),
    "nested_and_duplicate_intervals": case(
        [60], [(0, 10, 50), (0, 20, 30), (0, 20, 30), (0, 10, 50), (0, 49, 50)],
        answer([(0, 0, 10), (0, 50, 60)], [BAD_ENDS], [20], [(0, 10, 50)])),
}


def cut_case():
    """One piece a read, its ends bad: piece lengths 1 .. 40 eight times over and sixteen long ones, begins 0 .. 15 -- tests/test_scrub.py
    checks that the source offsets and the destination offsets of the pieces take every residue modulo 16 and that every length is there"""
    lengths, intervals, off = [], [], 0
    for i in range(336):
        ln = i % 40 + 1 if i < 320 else 100 + 13 * (i - 320)
        b = (i - off) % 16                                 # the piece starts at residue i % 16 of the read image
        lengths.append(b + ln + i % 3)
        intervals.append((i, b, b + ln))
        off += lengths[-1]
    return case(lengths, intervals, None, max_bad_permille=1000)


def load_shape_case(seed=3):
    """one read of 5 000 bases with 3 000 intervals beside 300 reads with one each"""
    rng = np.random.default_rng(seed)
    lengths, intervals = [200] * 150 + [5000] + [200] * 150, []
    for r, n in enumerate(lengths):
        for _ in range(3000 if n == 5000 else 1):
            b = int(rng.integers(0, n - 1))
            intervals.append((r, b, int(rng.integers(b + 1, min(b + 400, n) + 1))))
    return case(lengths, intervals, None, coverage=3)


CASES["cut_every_residue_and_length"] = cut_case()
CASES["one_read_with_thousands_of_intervals"] = load_shape_case()


def sweep(seed=20, count=36):
    """`count` random small sets over all parameters, from one seed"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 13))
        lengths = [int(rng.choice([0, 1, 2, int(rng.integers(3, 60)), int(rng.integers(60, 300))])) for _ in range(n)]
        intervals = []
        for r in range(n):                                                 # most reads are covered over most of their length, some deeply
            for _ in range(int(rng.integers(1, 9)) if lengths[r] and rng.random() < 0.8 else 0):
                b = int(rng.integers(0, max(lengths[r] // 8, 1)))
                intervals.append((r, b, int(rng.integers(max(lengths[r] - lengths[r] // 8, b + 1), lengths[r] + 1))))
        for _ in range(int(rng.integers(0, 61))):
            r = int(rng.integers(0, n))
            if lengths[r] == 0:
                continue
            b = int(rng.integers(0, lengths[r]))
            e = int(rng.integers(b + 1, lengths[r] + 1))
            if rng.random() < 0.3 and intervals:                       # shared endpoints are the rule among real overlaps
                r2, b2, e2 = intervals[int(rng.integers(0, len(intervals)))]
                r, b, e = r2, b2, int(rng.integers(b2 + 1, lengths[r2] + 1))
            intervals.append((r, b, e))
        c = case(lengths, intervals, None, coverage=int(rng.integers(0, 4)), max_bad_permille=int(rng.choice([0, 100, 400, 777, 1000])),
                 min_piece=int(rng.choice([1, 2, 10, 50])))
        c["with_reads"], c["with_quals"] = i % 3 != 2, i % 3 == 0
        out.append(c)
    return out
