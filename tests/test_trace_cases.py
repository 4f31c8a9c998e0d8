"""The case table of the stored band, the row records and the backtrack (tests/trace_cases.py) checked without a device: the restated band
against a brute-force scan, every claimed path against the oracle's pair list (vco_spoa_align_probe), every claimed in-degree, list
position and distance recomputed from the layers' own pair lists, the classification cap (no `unclear` alignment where band_redo is
asserted exactly), every in / out pair on its side of the band's edge, and the oracle time of the table.
tests/test_trace_cases_gpu.py runs the same table on the device."""
import os
import re

import pytest

import fwd_cases as fc
import trace_cases as tc

pytestmark = pytest.mark.usefixtures("built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = [c for c in tc.CASES if c.name[0] != "T"]


def _src(name):
    return open(os.path.join(ROOT, "vechat_amd", "csrc", name)).read()


def test_restated_constants_are_those_of_the_sources():
    """a tripwire, not a proof: the formulas and constants restated in trace_cases.py stand in the sources"""
    k, d, api = _src("vc_kernels.h"), _src("vc_device.h"), _src("vc_api.hip")
    assert "cpl >= 10u ? 8u : (cpl >= 8u ? 10u : (cpl >= 6u ? 14u : (uint32_t)VC_BAND_LANES))" in k
    assert "min((uint32_t)((((unsigned long long)len << 16) / nrows) / cpl), 0xFFFFFFu)" in k
    assert "const uint32_t t = __umul24(i, ql) >> 16;" in k and "return min(max(t, bl / 2u - 1u) - (bl / 2u - 1u), 64u - bl);" in k
    assert "return vc_band_start((r1 & ~(uint32_t)(VC_BAND_ROWS - 1)) + 1u + VC_BAND_ROWS / 2u, ql, bl);" in k
    for name, val, src in (("VC_BAND_ROWS", tc.VC_BAND_ROWS, k), ("VC_SPECW", tc.VC_SPECW, k), ("VC_BAND_LANES", tc.VC_BAND_LANES, d),
                           ("VC_INLINE_PRED", tc.VC_INLINE_PRED, d), ("VC_MAXTIE", tc.VC_MAXTIE, d), ("VC_KEPT", tc.VC_KEPT, api),
                           ("VC_BAND_CHAIN_COLS", 0, k)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), src), name
    assert re.search(r"#define VC_TW_WIN\s+%du\b" % tc.VC_TW_WIN, k)
    assert "bt->band = bt->packed && bt->kept;" in api and "bt->kept = (kKept && NC < 32768)" in api
    assert "if (kr - kp <= K) { hit = true;" in k and "d >= 2 && d <= 64 && d <= r" in k
    assert "|| d0 > 15u) ? 0u : d0" in k and "constexpr uint32_t ND_ = 3u;" in k


def test_band_at_its_bounds():
    assert [tc.band_lanes(c) for c in (4, 6, 8, 10, 12, 16, 24, 32)] == [16, 14, 10, 8, 8, 8, 8, 8]
    assert tc.band_slope(256, 256, 4) == 16384 and tc.band_slope(1 << 20, 1, 4) == 0xFFFFFF
    # left clamp: t <= bl/2 - 1 gives 0; right clamp: 64 - bl
    assert [tc.band_start(i, 16384, 16) for i in (1, 31, 32, 35, 36, 219, 220, 256)] == [0, 0, 1, 1, 2, 47, 48, 48]
    # the 24-bit multiply: only the low 24 bits of either operand count, and the low 32 bits of the product
    assert tc.band_start(1 << 24, 1 << 16, 8) == 0 and tc.band_start(0xFFFF, 0xFFFFFF, 8) == min(((0xFFFF * 0xFFFFFF) & 0xFFFFFFFF) >> 16, 59) - 3
    # a block of 16 rows shares the band of its 9th row
    assert {tc.band_row_start(r1, 16384, 16) for r1 in range(32, 48)} == {tc.band_start(41, 16384, 16)}
    assert tc.chain_walk(200) == (200, 200, 25) and tc.chain_walk(203) == (203, 203, 26)


@pytest.mark.parametrize("case", tc.CASES, ids=repr)
def test_sequences_fall_in_one_class_and_the_band_is_as_restated(case):
    assert case.seq_classes() == [case.classes[0]], case.seq_classes()
    assert case.banded() == (case.classes[0] < 32) and case.route()[1] == case.form
    assert all(2 <= len(w.seqs) - 1 for w in case.wins()) and 2 <= len(case.wins()) <= 4
    if not case.banded():
        return
    cpl = case.classes[0]
    bl = tc.band_lanes(cpl)
    for w in case.wins():
        band = tc.Band(len(w.seqs[-1]), w.L)                   # the probe's band
        starts = set()
        for r in range(1, w.L + 1):
            if (r - 1) % tc.VC_BAND_ROWS not in (0, tc.VC_BAND_ROWS - 1) and r != w.L:
                assert band.start(r) == band.start(r - 1)       # the band moves at block boundaries only
                continue
            cols = [c for c in range(1, 64 * cpl + 1) if band.in_band(r, c)]                                     # brute force, the first and last row of a block
            assert len(cols) == bl * cpl and cols == list(range(cols[0], cols[0] + bl * cpl)), (case, r)
            assert (cols[0] - 1) % cpl == 0 and 0 <= (cols[0] - 1) // cpl <= 64 - bl
            assert (r - 1) % tc.VC_BAND_ROWS == 0 or cols[0] == first
            first = cols[0]
            starts.add((cols[0] - 1) // cpl)
        assert 0 in starts                                      # the left clamp
        if len(w.seqs[-1]) > (64 - bl // 2) * cpl:
            assert 64 - bl in starts                            # the right clamp, where the probe reaches the last lanes


@pytest.mark.parametrize("case", CHAIN, ids=repr)
def test_paths_are_the_oracles_and_rows_are_backbone_positions(case):
    for wi, w in enumerate(case.wins()):
        built = [[] for _ in range(w.L + 1)]                  # in-edge lists recomputed from the layers' own pair lists
        for r in range(2, w.L + 1):
            built[r].append(r - 1)
        for k in range(1, len(w.seqs)):
            pairs, rank = tc.oracle_pairs(case, wi, k)
            assert list(rank) == list(range(w.L)), (case, wi, k)                          # rank -> node is the identity: row r is position r
            assert built == w.graph_for(k), (case, wi, k)
            assert tuple(tc.pairs_of(w.cells(k, case.scores))) == pairs, (case, wi, k, w.tag)
            nodes = [x for x, q in zip(pairs[0::2], pairs[1::2]) if x != -1 and q != -1]       # AddAlignment links the nodes that carry a base
            for a, b in zip(nodes, nodes[1:]):
                if a + 1 not in built[b + 1]:
                    built[b + 1].append(a + 1)


def _enter(cells, row):
    """(move, from row) by which the path enters `row`"""
    i = max(i for i, (r, c) in enumerate(cells) if r == row)
    (r, c), (pr, pc) = cells[i], cells[i + 1] if i + 1 < len(cells) else (0, 0)
    return ("diagonal" if pc == c - 1 else "vertical"), pr


def test_claimed_in_edges_and_moves():
    f = tc.BY_NAME["F15"]
    for wi, w in enumerate(f.wins()):
        g = w.graph_for(len(w.seqs) - 1)
        assert [301 - p for p in g[301]] == [1, 15, 16, 17] and all(len(g[r]) == 1 for r in range(2, w.L + 1) if r != 301)
        assert _enter(w.cells(len(w.seqs) - 1), 301) == ("diagonal", 301 - (15, 16, 17)[wi])      # in-edge 1, 2, 3 of the list
    for k in tc.IN_DEGREES:
        n = tc.BY_NAME[f"N{k}"]
        for wi, w in enumerate(n.wins()):
            g = w.graph_for(len(w.seqs) - 1)
            assert [101 - p for p in g[101]] == list(range(1, k + 1)) and (len(g[101]) > tc.VC_INLINE_PRED) == (k in (7, 9))
            assert _enter(w.cells(len(w.seqs) - 1), 101) == (("diagonal", "vertical")[wi], g[101][-1]), (k, wi)
    for s, w in zip(tc.JUMPS, tc.BY_NAME["W_run"].wins()):
        cells = w.cells(2)
        assert [c for r, c in cells if 20 <= r <= 20 + s] == [20] * (s + 1)              # the vertical run of s rows
    for name, sizes in (("W_jump32", tc.JUMPS), ("W_jump24", (200, 255))):
        for s, w in zip(sizes, tc.BY_NAME[name].wins()):
            g = w.graph_for(3)
            assert g[20 + s + 1] == [20 + s, 20] and all(len(g[r]) == 1 for r in range(2, w.L + 1) if r != 20 + s + 1)
            cells = w.cells(3)
            assert _enter(cells, 20 + s + 1) == ("diagonal", 20)                         # one step of s + 1 rows through the second in-edge
            assert len(cells) == w.L - s and 20 + s + 1 - 20 > tc.VC_TW_WIN - 64         # the window keeps at most 192 rows below the position
            assert [c for r, c in w.cells(2) if 20 <= r <= 20 + s] == [20] * (s + 1)     # the layer itself: a vertical run, it adds the edge
    for cpl in tc.BAND_CLASSES:                                                          # the clear window in the rows of the right clamp
        w = tc.BY_NAME[f"E{cpl}_del_in"].wins()[2]
        bl, L = tc.band_lanes(cpl), 64 * cpl
        p, cells, band = (64 - bl) * cpl + 2, w.cells(2), tc.Band(L, L)
        s = (L - p) // 2
        assert w.L == L == len(w.seqs[2]) and w.klass(2) == "clear"
        assert [c for r, c in cells if p <= r <= p + s] == [p] * (s + 1) and [r for r, c in cells if c > L - s] == [L] * s
        assert (p - 2) // cpl == 64 - bl and band.start(p + s) == 64 - bl and (L - 1) // cpl == 63      # first and last lane of the clamped band


def _kept_hit(g, L, r, p, K):
    """vc_frec_kept: does reader row r find predecessor row p in the ring?  (0-based record indices are rows - 1; the same arithmetic)"""
    kept = {q for x in range(1, L + 1) for q in g[x] if 2 <= x - q <= 64 and q >= 1}
    return 2 <= r - p <= 64 and len([q for q in kept if p <= q < r]) <= K


def test_kept_ring_claims():
    for name, far in (("R_d64", False), ("R_d65", True), ("R_k6", False), ("R_k7", True)):
        case = tc.BY_NAME[name]
        assert case.far == far and len(case.wins()) == 2
        for w in case.wins():
            g = w.graph_for(len(w.seqs) - 1)
            long = [(r, p) for r in range(1, w.L + 1) for p in g[r] if r - p > 2]
            assert len(long) == 1
            (r, p), = long
            assert r - p == {"R_d64": 64, "R_d65": 65}.get(name, 40)
            assert _kept_hit(g, w.L, r, p, tc.VC_KEPT) == (not far)
            if name[2] == "k":
                kept_between = [q for x in range(1, w.L + 1) for q in g[x] if x - q == 2]
                assert len(kept_between) == int(name[3:]) - 1 and all(p < q < r for q in kept_between)
            # every other read-back is served by the ring
            assert all(_kept_hit(g, w.L, x, q, tc.VC_KEPT) for x in range(1, w.L + 1) for q in g[x] if x - q == 2)


def test_classification_cap_and_pairs():
    groups = {}
    for case in tc.CASES:
        ks = [k for win in case.klasses() for k in win]
        if case.exact:
            assert "unclear" not in ks, (case, case.klasses())                           # the cap: 0 unclear alignments
        if case.group and case.group[0] == "E":
            groups.setdefault(case.group, {})[case.name.rsplit("_", 1)[1]] = case
    assert len(groups) == 2 * len(tc.BAND_CLASSES)
    for name, g in groups.items():
        assert g["in"].outside() == 0 and g["out"].outside() == len(g["out"].wins()) == 2, name
        assert len(g["in"].wins()) == (3 if name.endswith("del") else 2)                 # the clear window in the clamped rows (_e_lower)
        for wi, wo in zip(g["in"].wins(), g["out"].wins()):
            assert wi.L == wo.L and wi.klass(2) == "clear" and wo.klass(2) == "outside" and wi.klass(1) == wo.klass(1) == "clear"
            assert len(wi.seqs[2]) != len(wo.seqs[2])
    assert tc.BY_NAME["E32_raw"].outside() == 0 and not tc.BY_NAME["E32_raw"].banded()
    assert tc.BY_NAME["W_run"].outside() == 4 and tc.BY_NAME["W_jump24"].outside() == 4 and tc.BY_NAME["W_jump32"].outside() == 0
    assert tc.BY_NAME["W_jump24"].klasses() == (("clear", "outside", "outside"),) * 2 and not tc.BY_NAME["W_jump32"].banded()
    assert all(tc.BY_NAME[n].outside() == 0 for n in ("F15", "P_chain", "W_rows4", "W_rows6") + tuple(f"N{k}" for k in tc.IN_DEGREES))
    assert [[len(w.seqs) for w in c.wins()] for c in tc.CASES if c.name[0] == "T"] == [[n + 1] * 2 for n in tc.SINKS]


def test_the_oracle_polishes_every_window_and_its_time(capsys):
    """both overloads, and the pair lists of every layer (trace_steps); reports the oracle time of the whole table.  Timed around
    uncached calls, so that what ran earlier in the session does not shorten the figure."""
    t0 = fc.ORACLE_SECONDS[0]
    for case in tc.CASES:
        for mode in (0, 1):
            ref, pol, st = fc.oracle.__wrapped__(case, mode)
            assert all(pol) and all(len(r) > 0 for r in ref), (case, mode, pol)
        for wi, w in enumerate(case.wins()):
            for k in range(1, len(w.seqs)):
                assert len(tc.oracle_pairs.__wrapped__(case, wi, k)[0]) > 0
    dt = fc.ORACLE_SECONDS[0] - t0
    with capsys.disabled():
        print(f"\n[trace_cases] oracle time of the table, both overloads and every pair list: {dt:.1f} s (budget {tc.ORACLE_BUDGET:.0f} s)")
    assert dt < tc.ORACLE_BUDGET
