"""CPU suite: queries assigned to POA groups (vc_poa_run_assign, poa.poa_assign, the command line's --assign) at the boundary --
declared, exported and bound with the documented layout, the arguments refused before the device in the documented order, the
Python checks, the TSV writer -- and the two restated rules of tests/poa_assign_ref.py: the ranking, against the score tables of
tests/golden/poa_assign.json.gz (spoa's own Align of every query on every group's finished graph), and the row slots of
k_lg_slots, on hand-built graphs whose n_slots is worked out here."""
import ctypes as C
import gzip
import json
import os
import re

import numpy as np
import pytest

import poa_assign_ref as AR
from poa_common import _gp
from test_poa import _device_visible, load_fixture, members
from vechat_amd import capi, poa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_FX = {}


def load_assign_fixture():
    if not _FX:
        _FX.update(json.load(gzip.open(os.path.join(GOLDEN, "poa_assign.json.gz"), "rt")))
    return _FX


def entries():
    """every entry of the fixture -> [(name, groups as member lists, queries, (m, n, g, e, q, c), expected per algorithm)]"""
    named = {g["name"]: members(g) for g in load_fixture()["groups"]}
    return [(e["name"], [named[g] if isinstance(g, str) else members(g) for g in e["groups"]], [s.encode("latin-1") for s in e["queries"]],
             tuple(e["scores"]), e["expected"]) for e in load_assign_fixture()["entries"]]


def expected_assignments(groups, pairs, both_strands):
    """the fixture's pairs[k][w] = [score, score_rev] -> (table of kept scores, kept strands, per query (best, score, second, score))"""
    has_node = [any(len(s) for s, _ in g) for g in groups]
    both = [[AR.kept(a, b) if both_strands else (a, False) for a, b in row] for row in pairs]
    table = [[s for s, _ in row] for row in both]
    return table, [[r for _, r in row] for row in both], [AR.rank_pairs(row, has_node) for row in table]


# ------------------------------------------------------------------ the boundary
def test_assign_entry_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    assert "vc_poa_run_assign" in set(re.findall(r"\b(vc_[a-z_]+)\s*\(", hdr))
    assert "#define VC_POA_ASSIGN_STRANDS 1u" in hdr and "#define VC_POA_ASSIGN_SCORES  2u" in hdr
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libvechat_hip.so"))
    assert hasattr(lib, "vc_poa_run_assign")
    body = hdr[hdr.index("typedef struct vc_poa_assign_out"):hdr.index("} vc_poa_assign_out;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in capi.VcPoaAssignOut._fields_]
    assert C.sizeof(capi.VcPoaAssignOut) == 96 and capi.VcPoaAssignOut.n_queries.offset == 8 and capi.VcPoaAssignOut.n_groups.offset == 16
    assert capi.VcPoaAssignOut.status.offset == 24 and capi.VcPoaAssignOut.bytes.offset == 88
    assert capi.load_hip().vc_poa_run_assign.argtypes == [C.POINTER(capi.VcPoaGapParams), C.POINTER(capi.VcPoaGraphIn), C.POINTER(capi.VcBatch),
                                                          C.POINTER(capi.VcResult), C.POINTER(capi.VcBatch), C.POINTER(capi.VcPoaAssignOut)]
    assert (capi.VC_POA_ASSIGN_STRANDS, capi.VC_POA_ASSIGN_SCORES) == (1, 2)
    assert C.sizeof(capi.VcPoaAlignOut) == 80 and C.sizeof(capi.VcPoaGraphOut) == 152                                   # unchanged


def _call(lib, params, batch, qbatch, flags=0, out=True, queries=True, start=None, boverride=None, **qoverride):
    """-> (rc, the library's message, the assign output)"""
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)
    off = np.zeros(batch.n_windows + 1, np.uint64)
    status = np.zeros(max(batch.n_windows, 1), np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    vb.seq_begin = vb.seq_end = vb.win_fasta = None
    for k, v in (boverride or {}).items():
        setattr(vb, k, v)
    qv = qbatch.as_struct()
    qv.seq_begin = qv.seq_end = qv.win_fasta = qv.seq_has_qual = qv.quals = None
    for k, v in qoverride.items():
        setattr(qv, k, v)
    a = capi.VcPoaAssignOut(flags=flags)
    a.status = C.cast(1, C.POINTER(C.c_uint8))                                  # a failed call must leave every pointer NULL
    rc = lib.vc_poa_run_assign(C.byref(params) if params is not None else None, C.byref(start) if start is not None else None, C.byref(vb),
                               C.byref(r), C.byref(qv) if queries else None, C.byref(a) if out else None)
    return rc, lib.vc_poa_last_error().decode(), a


def test_assign_argument_errors_come_before_the_device_in_the_documented_order(built):
    lib = capi.load_hip()
    b = poa.group_batch([["ACGT", "ACGA"], [("AC", "II")]])
    q = poa.query_batch([["ACG", "AC", ""]])
    long_q = capi.Batch(np.array([0, 1], np.uint32), np.array([0, 65535], np.uint64), [0], [0], [0], np.zeros(65535, np.uint8) + 65,
                        np.zeros(65535, np.uint8), np.zeros(1, np.uint8))
    dec = (C.c_uint64 * 4)(0, 3, 2, 5)
    five = capi.VcPoaGraphIn(n_groups=5)
    # one defect each, in the documented order: q and a; as vc_poa_run_from with both (the parameters, the batch, the query batch and
    # its lengths, from); the flag bits
    bad = [("null assign output", lambda: _call(lib, _gp(), b, q, out=False), "both required"),
           ("null query batch", lambda: _call(lib, _gp(), b, q, queries=False), "both required"),
           ("null params", lambda: _call(lib, None, b, q), "null argument"),
           ("algorithm 3", lambda: _call(lib, _gp(algorithm=3), b, q), "algorithm"),
           ("gap_open > 0", lambda: _call(lib, _gp(gap_open=1), b, q), "opening"),
           ("match beyond int8", lambda: _call(lib, _gp(match=128), b, q), "-128..127"),
           ("batch offsets decrease", lambda: _call(lib, _gp(), b, q, boverride=dict(seq_off=dec)), "seq_off decreases"),
           ("query offsets decrease", lambda: _call(lib, _gp(), b, q, seq_off=dec), "query batch decreases"),
           ("null query bases", lambda: _call(lib, _gp(), b, q, bases=None), "null bases in the query batch"),
           ("query of 65 535 bases", lambda: _call(lib, _gp(), b, long_q), "query length"),
           ("five stored graphs for two groups", lambda: _call(lib, _gp(), b, q, start=five), "one graph per group"),
           ("unknown flag bit 4", lambda: _call(lib, _gp(), b, q, flags=4), "unknown assign flag")]
    for what, f, msg in bad:
        rc, text, a = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (what, rc, text)
        assert what == "null assign output" or (not a.status and not a.best_group and not a.scores), what   # (that call passes no output)
    # two defects: the earlier check answers
    order = [(lambda: _call(lib, _gp(algorithm=3), b, q, queries=False), "both required"),
             (lambda: _call(lib, _gp(algorithm=3), b, q, boverride=dict(seq_off=dec)), "algorithm"),
             (lambda: _call(lib, _gp(), b, long_q, boverride=dict(seq_off=dec)), "seq_off decreases"),
             (lambda: _call(lib, _gp(), b, long_q, start=five), "query length"),
             (lambda: _call(lib, _gp(), b, q, flags=8, start=five), "one graph per group"),
             (lambda: _call(lib, _gp(), b, q, flags=8, seq_off=dec), "query batch decreases")]
    for f, msg in order:
        rc, text, _ = f()
        assert rc == capi.VC_ERR_ARG and msg in text, (msg, rc, text)
    # the query batch's windows mean nothing: three windows for two groups pass the checks
    three = poa.query_batch([["A"], ["C"], ["G"]])
    if not _device_visible():                                                   # valid arguments reach the device check, and only then
        for kw in (dict(), dict(flags=1), dict(flags=3), dict(qbatch=three)):
            rc, text, a = _call(lib, _gp(), b, kw.pop("qbatch", q), **kw)
            assert rc == capi.VC_ERR_NO_DEVICE and not a.status, (kw, rc, text)


def test_assign_refuses_spans_and_weights_and_malformed_calls():
    with pytest.raises(ValueError, match="spans"):
        poa.poa_assign([["ACGT"]], ["ACG"], spans=[[None]])
    with pytest.raises(ValueError, match="weights"):
        poa.poa_assign([["ACGT"]], ["ACG"], weights=[[3]])
    with pytest.raises(ValueError, match="needs queries"):
        poa.poa_assign([["ACGT"]])
    with pytest.raises(ValueError, match="needs groups"):
        poa.poa_assign(queries=["ACG"])


def test_assign_tsv_writers():
    A = poa.Assignment
    res = [A(1, 40, 0, 12, False, capi.VC_WIN_OK), A(0, 7, -1, 0, True, capi.VC_WIN_INVALID), A(-1, 0, -1, 0, False, capi.VC_WIN_OVERFLOW)]
    assert poa.assign_tsv(["q1", b"q2", "q3"], ["a.fa", "b.fa"], res) == \
        b"q1\tb.fa\t40\ta.fa\t12\t+\tOK\nq2\ta.fa\t7\t*\t0\t-\tINVALID\nq3\t*\t0\t*\t0\t+\tOVERFLOW\n"
    assert poa.assign_scores_tsv(["q1", "q2"], ["a.fa", "b.fa"], np.array([[12, 40], [7, -3]], np.int32)) == \
        b"query\ta.fa\tb.fa\nq1\t12\t40\nq2\t7\t-3\n"


def test_command_line_refuses_assign_without_its_output(capsys):
    assert poa.main(["--assign", "q.fa", "x.fa"]) == 1 and "--assign-out" in capsys.readouterr().err
    assert poa.main(["--assign-scores", "s.tsv", "x.fa"]) == 1 and "--assign" in capsys.readouterr().err
    assert poa.main(["--assign", "q.fa", "--assign-out", "o.tsv", "--correct", "c.fa", "x.fa"]) == 1 and "--assign does not go" in capsys.readouterr().err


# ------------------------------------------------------------------ the ranking rule against the reference's score tables
def test_ranking_rule_on_hand_tables():
    assert AR.rank_pairs([], []) == (-1, 0, -1, 0)
    assert AR.rank_pairs([5], [True]) == (0, 5, -1, 0)
    assert AR.rank_pairs([5, 5, 5], [True] * 3) == (0, 5, 1, 5)                 # ties go to the lower index, twice
    assert AR.rank_pairs([1, 9, 9, 3], [True] * 4) == (1, 9, 2, 9)
    assert AR.rank_pairs([0, -7, -3], [False, True, True]) == (2, -3, 1, -7)    # an empty graph's 0 is scored, never ranked
    assert AR.rank_pairs([4, 8], [True, False]) == (0, 4, -1, 0)
    assert AR.query_status([0, 4, 2]) == AR.OVERFLOW and AR.query_status([0, 4]) == AR.INVALID and AR.query_status([]) == AR.OK
    assert AR.kept(3, 3) == (3, False) and AR.kept(3, 4) == (4, True) and AR.kept(0, -2) == (0, False)
    # the order in which groups arrive does not matter to the device's rule (a greater score, or an equal one from a lower group)
    scores = [3, 9, 9, 1, 9]
    for order in ([4, 3, 2, 1, 0], [2, 4, 0, 1, 3]):
        bg, bs, sg, ss = -1, 0, -1, 0
        for w in order:
            s = scores[w]
            if bg < 0 or s > bs or (s == bs and w < bg):
                bg, bs, sg, ss = w, s, bg, bs
            elif sg < 0 or s > ss or (s == ss and w < sg):
                sg, ss = w, s
        assert (bg, bs, sg, ss) == AR.rank_pairs(scores, [True] * 5)


def test_fixture_can_fail_and_the_ranking_reproduces_it():
    seen = dict(not_group_0=False, tie=False, reversed_kept=False, strands_differ=False, empty_group_scored_not_ranked=False)
    n = 0
    for name, groups, queries, scores, exp in entries():
        for t in ("0", "1", "2"):
            pairs = exp[t]["pairs"]
            assert len(pairs) == len(queries) and all(len(row) == len(groups) for row in pairs), (name, t)
            for strands in (False, True):
                table, rev, ranks = expected_assignments(groups, pairs, strands)
                for k, (bg, bs, sg, ss) in enumerate(ranks):
                    n += 1
                    ranked = [w for w, g in enumerate(groups) if any(len(s) for s, _ in g)]
                    assert (bg in ranked and sg in ranked and bg != sg) if len(ranked) > 1 else sg == -1, (name, t, k)
                    if bg >= 0:                                                 # the definition, in the plainest words
                        assert bs == max(table[k][w] for w in ranked) and bg == min(w for w in ranked if table[k][w] == bs)
                    if sg >= 0:
                        rest = [w for w in ranked if w != bg]
                        assert ss == max(table[k][w] for w in rest) and sg == min(w for w in rest if table[k][w] == ss)
                    seen["not_group_0"] |= bg > 0
                    seen["tie"] |= sg >= 0 and bs == ss
                    seen["reversed_kept"] |= strands and bg >= 0 and rev[k][bg]
                    seen["strands_differ"] |= strands and sg >= 0 and rev[k][bg] != rev[k][sg]
                    seen["empty_group_scored_not_ranked"] |= any(w not in ranked and table[k][w] == 0 > bs for w in range(len(groups)))
    assert all(seen.values()) and n == 6 * sum(len(q) for _, _, q, _, _ in entries()) > 0, (seen, n)


# ------------------------------------------------------------------ the slot rule on hand-built graphs
# n_slots by hand (slot 0 is row 0's for good; a row's slot comes back only when the last row that reads it is complete):
#   chain            row 1 takes 1; row 2 takes 2 and frees 1; row 3 takes 1 and frees 2; ...: 3
#   one bubble       1 -> {2, 3} -> 4: rows 1, 2, 3 hold 1, 2, 3 (row 1 until row 3 is complete), row 4 takes 1: 4
#   skip edge        the chain's three, and row 1 stays alive until the last row reads it: 4
#   in-degree 9      the source, its 9 successors side by side, the source's slot free for the join: 1 + 1 + 9 = 11
#   wide             20 sources side by side, then each column shifts by one slot: 1 + 20 + 1 = 22
#   one node         row 0 and the node: 2
@pytest.mark.parametrize("name", sorted(AR.HAND_ROWS))
def test_slot_rule_on_hand_built_graphs(name):
    preds, want = AR.HAND_ROWS[name]
    assert want == {"chain": 3, "one_bubble": 4, "skip_edge_first_to_last": 4, "in_degree_9": 11, "wide_20_chains": 22, "one_node": 2}[name]
    slot, n_slots = AR.slots(preds)
    assert n_slots == want, (name, slot)
    AR.check_slots(preds, slot, n_slots)
    assert slot[0] == 1 and 0 not in slot                                       # the lowest free slot; row 0's is never given out
    if name == "skip_edge_first_to_last":
        assert slot.count(slot[0]) == 1                                         # row 1 stays alive throughout: nobody else uses its slot
    if name == "in_degree_9":
        assert slot[-1] == 1 and sorted(slot[1:10]) == list(range(2, 11))
    if name == "chain":
        assert slot == [1, 2, 1, 2, 1]


def test_slot_rule_keeps_its_invariant_on_random_graphs():
    import random
    rng = random.Random(11)
    for _ in range(200):
        n = rng.randint(1, 40)
        preds = [sorted(rng.sample(range(1, r + 1), min(r, rng.choice([0, 1, 1, 1, 2, 3])))) if r else [] for r in range(n)]
        slot, n_slots = AR.slots(preds)
        AR.check_slots(preds, slot, n_slots)
        assert n_slots <= n + 1


def test_check_slots_refuses_a_shared_slot():
    preds, _ = AR.HAND_ROWS["one_bubble"]
    with pytest.raises(AssertionError):
        AR.check_slots(preds, [1, 2, 2, 1], 3)                                  # rows 2 and 3 are both read by row 4
    with pytest.raises(AssertionError):
        AR.check_slots(preds, [1, 2, 3, 2], 4)                                  # row 4 on the slot of a row it reads
