"""CPU tests of tests/align_ref.py, the restatement that pins the overlap aligner's path (tests/test_align.py compares the device's
CIGAR strings with it).  The restatement is held against answers derived by hand from the tie-break rule -- diagonal, then insertion,
then deletion, from the end -- and, on seeded random pairs, against an independent two-row DP and a walk of its own CIGARs."""
import random

import pytest

import align_ref as ar

# (q, t, cigar, distance), worked out by hand from the rule; not taken from the device code
KNOWN = [
    (b"AAA", b"AAAAA", "2D3M", 2),
    (b"AAAAA", b"AAA", "2I3M", 2),
    (b"AAA", b"CCCCC", "2D3M", 5),
    (b"ACGT", b"A", "1M3I", 3),
    (b"A", b"ACGTACGT", "4D1M3D", 7),
    (b"ACAC", b"AC", "2I2M", 2),
    (b"AC", b"ACAC", "2D2M", 2),
    (b"AG", b"GA", "2M", 2),
    (b"ACGT", b"AGT", "1M1I2M", 1),
    (b"", b"ACG", "3D", 3),
    (b"ACG", b"", "3I", 3),
    (b"", b"", "", 0),
]


@pytest.mark.parametrize("q,t,cigar,dist", KNOWN, ids=[f"{q.decode() or '-'}_{t.decode() or '-'}" for q, t, _, _ in KNOWN])
def test_known_answers(q, t, cigar, dist):
    assert ar.align(q, t) == (cigar, dist)


def test_bytes_compare_as_bytes():
    assert ar.align(b"acgt", b"ACGT") == ("4M", 4)                  # case matters
    assert ar.align(b"ANA", b"ANA") == ("3M", 0) and ar.align(b"ANA", b"ACA")[1] == 1      # N equals only N
    assert ar.align(b"\xff\x00\xff", b"\xff\x00\xff") == ("3M", 0)


def random_pairs():
    """a few hundred seeded pairs, lengths 0..300: ACGT, two letters (ties everywhere), the full byte range; related and unrelated"""
    rng = random.Random(20240)
    pairs = []
    for alphabet in (b"ACGT", b"AC", bytes(range(256))):
        for _ in range(100):
            n, m = rng.randint(0, 300), rng.randint(0, 300)
            t = bytes(rng.choice(alphabet) for _ in range(m))
            if rng.random() < 0.5:                                  # q: a slice of t with edits, so that the path has long diagonals
                lo = rng.randint(0, m); hi = rng.randint(lo, m)
                q = bytearray(t[lo:hi])
                for _ in range(rng.randint(0, 12)):
                    p = rng.randint(0, len(q))
                    r = rng.random()
                    if r < 0.3:
                        del q[p:p + rng.randint(1, 4)]
                    elif r < 0.6:
                        q[p:p] = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 4)))
                    elif p < len(q):
                        q[p] = rng.choice(alphabet)
                q = bytes(q)
            else:
                q = bytes(rng.choice(alphabet) for _ in range(n))
            pairs.append((q, t))
    return pairs


def test_random_pairs_distance_walk_and_gap_order():
    for q, t in random_pairs():
        cigar, dist = ar.align(q, t)
        assert dist == ar.two_row_distance(q, t), (len(q), len(t))
        assert ar.cigar_cost(cigar, q, t) == dist, (len(q), len(t), cigar[:60])
        # Never a D next to an I, in either order.  Both gaps together go from (i-1, j-1) to (i, j) at cost 2, and each was taken because
        # its cell is its neighbour's + 1, so D[i][j] = D[i-1][j-1] + 2; the diagonal bounds D[i][j] by D[i-1][j-1] + 1: contradiction.
        assert "DI" not in _ops_only(cigar) and "ID" not in _ops_only(cigar), cigar[:60]


def _ops_only(cigar):
    return "".join(c for c in cigar if c in "MID")


def test_cigar_cost_rejects_what_is_not_an_alignment():
    assert ar.cigar_cost("3M", b"ACG", b"ACG") == 0
    assert ar.cigar_cost("2M", b"ACG", b"ACG") is None              # leaves a base over
    assert ar.cigar_cost("4M", b"ACG", b"ACG") is None              # runs past the end
    assert ar.cigar_cost("3M1I", b"ACG", b"ACG") is None
    assert ar.cigar_cost("3X", b"ACG", b"ACG") is None
    assert ar.cigar_cost("0I3M", b"ACG", b"ACG") is None
    assert ar.cigar_cost("", b"", b"") == 0
