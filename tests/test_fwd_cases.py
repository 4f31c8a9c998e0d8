"""The forward pass's case table (tests/fwd_cases.py) checked without a device: every case's sequences fall in the width classes it
claims, the 21 instantiations of launch_fwd are each named once, the restated routing gives the claimed kernel form, every pair of
envelope cases lands on opposite sides of its predicate, the oracle polishes every window of every case in both overloads, and a plain
int64 DP says how close each envelope case gets to its bound.  tests/test_fwd_classes_gpu.py runs the same table on the device."""
import os
import re

import pytest

import fwd_cases as fc

pytestmark = pytest.mark.usefixtures("built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = [c for c in fc.CASES if c.name[0] == "A"]
B = [c for c in fc.CASES if c.name[0] == "B"]
C_ = [c for c in fc.CASES if c.name[0] == "C"]
D = [c for c in fc.CASES if c.name[0] == "D"]


def _src(name):
    return open(os.path.join(ROOT, "vechat_amd", "csrc", name)).read()


def test_restated_constants_are_those_of_the_sources():
    """a tripwire, not a proof: the bounds and the class list restated in fwd_cases.py stand in the C predicates, and each predicate names
    the file"""
    k, d = _src("vc_kernels.h"), _src("vc_fwd_dt.h")
    body = lambda s, name: s[s.index(name):s.index("}", s.index("return", s.index(name)))]
    assert "{4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64}" in body(k, "uint32_t vc_cpl_for(") and list(fc.CLASSES) == [4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64]
    assert "(cpl - 1) * ((m > n ? m : n) - 2 * g) <= 255" in body(k, "bool vc_row_packed(")
    assert "lo >= -31744 && (m - g) * (64 * cpl + 1) < 32767" in body(k, "bool vc_int16_ok(")
    assert "mm * cols + (nrows + cols + 8) * (-g) <= 65000" in body(d, "bool vc_dt_ok(")
    assert "(cpl + 2 + 3) / 4" in k[k.index("constexpr int vc_nds("):][:80]
    for s, name in ((k, "vc_cpl_for("), (k, "vc_row_packed("), (k, "vc_int16_ok("), (d, "vc_dt_ok(")):
        at = s.index("inline " + ("uint32_t " if "cpl_for" in name else "bool ") + name)
        assert "tests/fwd_cases.py" in s[at - 300:at], name
    api = _src("vc_api.hip")
    assert re.search(r"const bool dt = c->dt && bt->packed && bt->cpl < 32 && vc_dt_ok\(", api) and "if (hi - lo > 1) { lo = hi - 1; a.fold = 1; }" in api
    assert "if (cpl >= 32 && bt->lean != 3u) maybe_wide = true;" in api and "est = depth > 0 ? 0.33 * ((double)sum / depth) * std::pow(depth, 0.55)" in api


def test_predicates_at_their_bounds():
    assert [fc.cpl_for(x) for x in (1, 256, 257, 384, 385, 1536, 1537, 2048, 2049, 4096, 4097)] == [4, 4, 6, 6, 8, 24, 32, 32, 48, 64, 0]
    assert fc.spread_bound(3, -5, -4, 24) == 253 and fc.row_packed(3, -5, -4, 24) and not fc.row_packed(3, -5, -4, 32)
    assert fc.dt_ok(4, -6, -16, 3413, 8) and not fc.dt_ok(4, -6, -16, 3414, 8)
    assert fc.int16_ok(60, -10, -67, 465, 4, True) and not fc.int16_ok(60, -10, -67, 466, 4, True) and not fc.int16_ok(61, -10, -67, 100, 4, False)
    assert [fc.nds(c) for c in fc.CLASSES] == [2, 2, 3, 3, 4, 5, 6, 7, 9, 13, 17]


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_sequences_fall_in_the_claimed_classes(case):
    cls = case.seq_classes()
    assert (cls[0], cls[-1]) == case.classes, cls
    if case.name[0] == "A" or case.name[0] == "D":
        assert cls == [case.classes[0]]                        # every sequence, backbone included
    if case.name[0] == "B":
        ca, cb = case.classes
        assert cls == [ca, cb]
        w0, w1 = case.windows()
        assert {fc.cpl_for(len(s)) for s in w1[0]} == {ca}                              # the second window lies entirely in CA
        assert sorted(len(s) - 64 * ca for s in w0[0])[0] == -1 and max(len(s) - 64 * ca for s in w0[0]) == 2     # straddles the edge by 1 .. 2 columns
    if case.name[0] == "C":
        assert len(cls) > 2 and cls[-2:] == list(case.inst[1:]), cls                    # hi - lo > 1, full-span layers in the two widest classes
        for w in case.windows():
            assert sorted(len(s) for s, b, e in zip(w[0], w[2], w[3]) if not fc.full_span(b, e, len(w[0][0])))[:3] == [100, 300, 700]
    for w in case.windows():
        assert 4 <= len(w[0]) or case.name.startswith("D"), len(w[0])


def test_edge_lengths_of_every_class():
    """A: reads of exactly 64 * CPL columns and of 64 * CPL_prev + 1, per class"""
    for case in A:
        cpl = case.classes[0]
        lens = {len(s) for w in case.windows() for s in w[0]}
        assert 64 * cpl in lens and 64 * fc._prev(cpl) + 1 in lens and 64 * cpl - 1 in lens, (case, sorted(lens))


def test_all_21_instantiations_are_named_once():
    named = [c.inst for c in A + B]
    want = [(c, c) for c in fc.CLASSES] + list(fc.PAIRS)
    assert sorted(named) == sorted(want) and len(set(named)) == 21
    assert [c.inst for c in C_] == [("fold", 20, 24), ("fold", 24, 32), ("fold", 48, 64)]


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_route_gives_the_claimed_instantiation_and_form(case):
    inst, form, wide = case.route()
    assert (inst, form) == (case.inst, case.form), (inst, form, wide)
    if form == "dt":
        assert case.route(vc_dt=False)[1] == "packed"
    # default scores: class 24 is the last packed / dt class, class 32 the first raw one (the boundary of the shipped parameters)
    if case.scores is fc.DEFAULT:
        assert form == ("dt" if case.classes[1] <= 24 else "raw") and not wide


def test_every_envelope_pair_is_split_by_its_predicate():
    groups = {}
    for c in D:
        groups.setdefault(c.group, []).append(c)
    assert sorted(groups) == ["D16", "D255_c16", "D255_c4", "D255_c6", "Ddt"] and all(len(g) == 2 for g in groups.values())
    for name, (a, b) in groups.items():
        assert a.windows() == b.windows(), name                  # the same sequences on both sides
        assert a.route()[1] != b.route()[1], name
    for cpl in (16, 6, 4):
        a, b = groups[f"D255_c{cpl}"]
        assert fc.spread_bound(*a.scores.key(), cpl) == 255 and fc.spread_bound(*b.scores.key(), cpl) > 255
        assert (a.route()[1], b.route()[1]) == ("dt", "raw")
    a, b = groups["Ddt"]
    assert fc.dt_top(4, -16, a.nc(), 8) <= 65000 < fc.dt_top(4, -16, b.nc(), 8) and (a.nc(), b.nc()) == fc.DT_NC and b.nc() - a.nc() == 64
    assert (a.route()[1], b.route()[1]) == ("dt", "packed")
    a, b = groups["D16"]
    assert fc.int16_cols(60, -67, 4) == 32639 < 32767 <= fc.int16_cols(61, -67, 4) == 32896
    assert (a.route(), b.route()) == (((4, 4), "raw", False), ((4, 4), "wide-only", True))
    assert fc.int16_ok(60, -10, -67, a.nc(), 4, True)             # the global rows pass lo >= -31 744 with dec = 67


def test_the_oracle_polishes_every_window_of_every_case(capsys):
    """both overloads; no case may be dropped from this loop.  Reports the oracle time of the whole table."""
    for case in fc.CASES:
        for mode in (0, 1):
            ref, pol, st = fc.oracle(case, mode)
            assert all(pol) and all(len(r) > 0 for r in ref), (case, mode, pol)
    with capsys.disabled():
        print(f"\n[fwd_cases] oracle time of the table, both overloads: {fc.ORACLE_SECONDS[0]:.1f} s")
    assert fc.ORACLE_SECONDS[0] < 60


def test_the_dt_case_fills_its_capacity():
    """the oracle's graph at the end of the build (the largest the forward pass meets) has >= 90 % of the dt-side capacity in rows and fits it"""
    import oracle_api as oa
    case = fc.BY_NAME[f"Ddt_nc{fc.DT_NC[0]}"]
    rows = max(s[2] for s in oa.oracle_stages(case.batch(), case.params(0), 0))
    assert rows == fc.DT_ROWS == fc.oracle(case, 0)[2]["max_nodes"]
    assert 0.9 * fc.DT_NC[0] <= rows <= fc.DT_NC[0]
    assert len(case.windows()[0][0]) - 1 == fc.DT_DEPTH
    # the top cells then approach the bound: T'' of the last row's last column is H + (rows + columns) * 16 with H >= (rows + columns) * g
    assert (rows + 512) * 16 > 0.9 * 65000


def _probe(case, k):
    w = case.windows()[0]
    L = len(w[0][0])
    local = not fc.full_span(w[2][k], w[3][k], L)
    return local, fc.tilted_extremes(w[0][0], w[0][k], *case.scores.key(), case.classes[1], local)


def test_envelope_attainment(capsys):
    """Plain int64 DP of one layer against the backbone (a chain graph, so ordinary NW / SW) in the kernels' tilted forms.  Layer 1 only:
    what later layers attain against the branching graph is not computed on the CPU.  Each value stays inside the bound on the side that
    claims it, the byte-packed cases attain their 255 exactly, and the table in fwd_cases.ATTAINED is what this computes."""
    got = {}
    for case in D:
        local, x = _probe(case, 1)
        got[case.name] = dict(local=local, **x)
        if case.form == "dt":
            assert x["spread"] <= 255 and x["t2_max"] <= 65535 and x["t_min"] >= -31744 and x["t_max"] <= 32767, (case, x)
        if case.group.startswith("D255"):
            if case.form == "dt":
                assert x["spread"] >= 128, (case, x)             # (at least half the bound, or the events need strengthening: it is all of it)
            else:
                assert x["spread"] > 255, (case, x)              # the neighbour really needs the raw form
                assert x["t_min"] >= -31744 and x["t_max"] <= 32767
    # vc_int16_ok's column bound: the local alignment of the piece that equals the backbone reaches (m - g) * 256
    assert got["D16_m60"]["local"] and got["D16_m60"]["t_max"] == 127 * 256 <= 32767 and got["D16_m60"]["t_min"] >= 0
    assert got["D16_m61"]["t_max"] == 128 * 256 > 32767                  # one more and int16 would not hold it: k_fwd_wide's side
    local, g2 = _probe(fc.BY_NAME["D16_m60"], 2)                         # a global layer of the same window: rows, with dec = 67
    assert not local and -31744 <= g2["t_min"] and g2["t_max"] <= 32767
    got["D16_m60 (layer 2, global)"] = dict(local=False, **g2)
    with capsys.disabled():
        print("\n[fwd_cases] attained on layer 1 (bounds: spread 255, T'' 65 535, T -31 744 .. 32 767)")
        for k, v in got.items():
            print(f"  {k:28s} {'local ' if v['local'] else 'global'} spread {v['spread']:4d}  T'' max {v['t2_max']:6d}  T min {v['t_min']:7d}  T max {v['t_max']:6d}")
    assert {k: (v["spread"], v["t2_max"], v["t_min"], v["t_max"]) for k, v in got.items()} == fc.ATTAINED
