"""Generates tests/golden/poa_align.json.gz: queries aligned against the finished graphs of POA groups without being added
(vc_poa_run_align, vechat_amd.poa.poa_align) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the
reference tree lies (REF, as in oracle/Makefile).  The few lines of C++ below -- this generator's own -- are compiled in a
temporary directory against spoa's public headers and linked to oracle/_ref/libvcref_sisd.so (the SIMD build libvcref_sse41.so
compared: simd_agrees; the scalar build is the bar): the plain build loop of spoa's command line, then per query
`engine->Align(query, graph, &score)`, and with strands the comparison of src/main.cpp:287-304 without the add.  Nothing built
is kept.

  python tests/golden/make_poa_align.py

Every entry has the group, its `queries`, `flips` (the queries reverse-complemented -- by the test, with
tests/poa_strand_ref.reverse_complement -- before the strand run), `plain` (every query as given) and `strand` (both strands);
a result is tests/poa_align_ref.pack's [score, score_rev, reversed, pairs, first differences of nodes and positions], or the
SHA-256 of the pairs where an entry has more than FULL of them.
  kat     the 18 score sets of spoa_kat_gaps.json: the graph of the first 40 reads of sample.fastq.gz, the other 15 as queries,
          every second one flipped for the strand run;
  groups  the 30 seeded groups of poa_groups.json.gz at the three algorithms, four queries each: a member, a mutated member,
          a random sequence, a member reverse-complemented;
  gaps    five of them at one affine and one convex score set;
  hand    the hand-made groups below.
Asserted here, so that the fixture can fail: an entry keeps a reversed query; one has a tie (score == score_rev) on a non-empty
alignment, kept as given; under affine gaps one has a gap run of at least 2 in each direction; one has both kinds of -1; one
local entry is empty.
"""
import ctypes as C
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fixtures  # noqa: E402
import poa_align_ref as A  # noqa: E402
from poa_strand_ref import reverse_complement  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SPOA = os.path.join(REF, "vendor", "spoa")
TYPES = {"SW": 0, "NW": 1, "OV": 2}
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")
FULL = 4000                            # pairs of an entry (both runs) up to which they are kept in full
FULL_KAT = ("GlobalAffine",)           # ... and one known answer, whatever its size

HARNESS = r"""
#include <atomic>
#include <cstdint>
#include <exception>
#include <memory>
#include <string>
#include <vector>
#include "biosoup/sequence.hpp"
#include "spoa/spoa.hpp"

std::atomic<std::uint32_t> biosoup::Sequence::num_objects{0};

// out, per query: score, score_rev, reversed, pairs, then (node, position) per pair.  Returns the count; -1: the reference threw;
// -2: out is too small
extern "C" int64_t align_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, uint32_t nq,
                             const char* const* qseqs, const uint32_t* qlens, int type, int m, int n, int g, int e, int q, int c,
                             int strands, int64_t* out, int64_t cap) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        spoa::Graph graph{};
        for (uint32_t i = 0; i < k; ++i) {
            std::string s(seqs[i], lens[i]);
            auto alignment = engine->Align(s, graph);
            if (quals[i]) graph.AddAlignment(alignment, s, std::string(quals[i], lens[i]));
            else graph.AddAlignment(alignment, s);
        }
        std::vector<int64_t> v;
        for (uint32_t i = 0; i < nq; ++i) {
            biosoup::Sequence it("q", 1, qseqs[i], qlens[i]);
            std::int32_t score = 0, score_rev = 0;
            auto alignment = engine->Align(it.data, graph, &score);
            int64_t reversed = 0;
            if (strands) {
                it.ReverseAndComplement();
                auto alignment_rev = engine->Align(it.data, graph, &score_rev);
                if (!(score >= score_rev)) { alignment = alignment_rev; reversed = 1; }
            }
            v.push_back(score); v.push_back(score_rev); v.push_back(reversed); v.push_back(alignment.size());
            for (const auto& p : alignment) { v.push_back(p.first); v.push_back(p.second); }
        }
        if ((int64_t)v.size() > cap) return -2;
        for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
        return v.size();
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_reference(tmp):
    src = os.path.join(tmp, "align_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    inc = [x for d in ("include", "src", "vendor/cereal/include", "vendor/bioparser/include", "vendor/bioparser/vendor/biosoup/include")
           for x in ("-I", os.path.join(SPOA, d))]
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"align_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, src, "-o", out, so, "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].align_run.restype = C.c_int64
    return libs


def run(lib, members, queries, atype, scores, strands):
    """-> [align_one()-shaped dict per query], from the reference"""
    k, nq = len(members), len(queries)
    SA, QA = C.c_char_p * max(k, 1), C.c_char_p * max(nq, 1)
    cap = 64 + sum(4 + 2 * (len(s) + sum(len(x) for x, _ in members)) for s in queries)
    out = (C.c_int64 * cap)()
    n = lib.align_run(C.c_uint32(k), SA(*[s for s, _ in members]), (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members]),
                      SA(*[q for _, q in members]), C.c_uint32(nq), QA(*queries), (C.c_uint32 * max(nq, 1))(*[len(s) for s in queries]),
                      C.c_int(atype), *[C.c_int(x) for x in scores], C.c_int(1 if strands else 0), out, C.c_int64(cap))
    assert n >= 0, n
    v, at, res = list(out[:n]), 0, []
    for _ in range(nq):
        sc, scr, rev, npairs = v[at:at + 4]
        at += 4
        res.append(dict(score=sc, score_rev=scr if strands else None, reversed=bool(rev),
                        pairs=[[v[at + 2 * i], v[at + 2 * i + 1]] for i in range(npairs)]))
        at += 2 * npairs
    assert at == n
    return res


CHECK = []                             # (type, scores, strands, results, queries as run) of every run, for the assertions at the end


def entry(libs, members, queries, flips, atype, scores, full=False):
    fl = set(flips)
    squeries = [reverse_complement(s) if i in fl else s for i, s in enumerate(queries)]
    plain, strand = run(libs["sisd"], members, queries, atype, scores, False), run(libs["sisd"], members, squeries, atype, scores, True)
    simd = run(libs["sse41"], members, queries, atype, scores, False) == plain and \
        run(libs["sse41"], members, squeries, atype, scores, True) == strand
    CHECK.append((atype, scores, False, plain, queries))
    CHECK.append((atype, scores, True, strand, squeries))
    full = full or sum(len(r["pairs"]) for r in plain + strand) <= FULL
    return dict(plain=[A.pack(r, full) for r in plain], strand=[A.pack(r, full) for r in strand], simd_agrees=simd)


def mutate(rng, s, rate=0.08):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= x < rate:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def four_queries(rng, members):
    """a member, a mutated member, a random sequence, a member reverse-complemented"""
    nonempty = [s for s, _ in members if s] or [b"ACGTTGCA"]
    a, b, c = rng.choice(nonempty), rng.choice(nonempty), rng.choice(nonempty)
    return [a, mutate(rng, b) or b[:1], bytes(rng.choice(b"ACGT") for _ in range(max(1, len(a)))), reverse_complement(c)]


def hand_groups():
    """[(name, [(sequence, quality or None)], [query], flips)]"""
    rng = random.Random(20250301)
    R = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))            # noqa: E731
    base = R(80)
    grp = [(base, None), (mutate(rng, base), None), (mutate(rng, base), None)]
    pal = b"ACGTTGCATGCAACGT"                                             # its own reverse complement
    assert reverse_complement(pal) == pal
    gap_base = R(60)
    return [
        ("empty_query", grp, [b"", base, b""], []),
        ("queries_for_an_empty_group", [], [base, b"", b"A"], [0]),
        ("queries_for_empty_members_only", [(b"", None), (b"", None)], [base], []),
        ("byte_outside_the_graphs_alphabet", grp, [base[:40] + b"N" + base[41:], b"NNNN", base[:10] + b"acgt" + base[14:]], []),
        ("local_finds_nothing", [(b"AAAAAAAAAAAAAAAAAAAA", None), (b"AAAAAAAAAAAAAAAAAAA", None)], [b"CCCCCCCCCC", b"GGGGG", b"AAAA"], []),
        ("query_of_length_1", grp, [base[:1], base[40:41], b"N"], []),
        ("query_longer_than_every_path", grp, [R(25) + base + R(30), base + base], [1]),
        ("reverse_palindrome_tie", [(pal, None), (pal, None)], [pal, pal[:8] + pal[8:]], []),
        # deletions and insertions of several bases between matching flanks: gap runs of at least 2 in both directions
        ("gap_runs", [(gap_base, None), (gap_base, None), (gap_base, None)],
         [gap_base[:20] + gap_base[26:], gap_base[:30] + b"TTTTTT" + gap_base[30:], gap_base[:15] + gap_base[19:40] + b"GGGG" + gap_base[40:]], [2]),
    ]


def main():
    seqs, quals = fixtures.load_sample_reads()
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_reference(tmp)
        kat = {}
        for name, k in json.load(open(os.path.join(HERE, "spoa_kat_gaps.json"))).items():
            members = list(zip(seqs[:40], quals[:40] if k["quality"] else [None] * 40))
            queries = list(seqs[40:])
            scores = (k["m"], k["n"], k["g"], k["e"], k["q"], k["c"])
            flips = list(range(1, len(queries), 2))
            kat[name] = dict(type=k["type"], scores=list(scores), quality=k["quality"], flips=flips,
                             **entry(libs, members, queries, flips, TYPES[k["type"]], scores, name in FULL_KAT))
        rng = random.Random(20250302)
        groups, by_name = [], {}
        for g in poa_fx["groups"]:
            members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
            queries = four_queries(rng, members)
            by_name[g["name"]] = (members, queries)
            m, n, gp = g["scores"]
            exp = {t: entry(libs, members, queries, [], int(t), (m, n, gp, gp, gp, gp)) for t in ("0", "1", "2")}
            groups.append(dict(name=g["name"], scores=[m, n, gp], queries=[s.decode("latin-1") for s in queries], flips=[], expected=exp))
        gaps = []
        for name in GAP_GROUPS:
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                members, queries = by_name[name]
                exp = {t: entry(libs, members, queries, [], int(t), scores) for t in ("0", "1", "2")}
                gaps.append(dict(name=name, model=model, scores=list(scores), queries=[s.decode("latin-1") for s in queries], flips=[],
                                 expected=exp))
        hand = []
        for name, members, queries, flips in hand_groups():
            for model, scores in (("linear", (5, -4, -8, -8, -8, -8)), ("affine", (5, -4, -8, -6, -8, -6))):
                exp = {t: entry(libs, members, queries, flips, int(t), scores, True) for t in ("0", "1", "2")}
                hand.append(dict(name=name, model=model, scores=list(scores), seqs=[[s.decode(), q] for s, q in members],
                                 queries=[s.decode("latin-1") for s in queries], flips=flips, expected=exp))

    # the fixture can fail
    def runs(pairs, side):
        best = cur = 0
        for p in pairs:
            cur = cur + 1 if p[side] == -1 else 0
            best = max(best, cur)
        return best
    assert any(r["reversed"] for _, _, st, res, _ in CHECK if st for r in res), "no reversed query kept"
    assert any(r["score"] == r["score_rev"] and r["pairs"] and not r["reversed"] for _, _, st, res, _ in CHECK if st for r in res), "no tie"
    aff = [r for _, sc, _, res, _ in CHECK if sc[2] < sc[3] and (sc[2] <= sc[4] or sc[3] >= sc[5]) for r in res]
    assert any(runs(r["pairs"], 0) >= 2 for r in aff) and any(runs(r["pairs"], 1) >= 2 for r in aff), "no affine gap run of 2 in each direction"
    assert any(runs(r["pairs"], 0) and runs(r["pairs"], 1) for _, _, _, res, _ in CHECK for r in res), "no alignment with both kinds of -1"
    assert any(not r["pairs"] and r["score"] == 0 and len(q) for t, _, _, res, qs in CHECK if t == 0 for r, q in zip(res, qs)), "no empty SW entry"
    every = [e for k in kat.values() for e in (k,)] + [g["expected"][t] for g in groups + gaps + hand for t in ("0", "1", "2")]
    fx = dict(params=dict(generator="tests/golden/make_poa_align.py",
                          reference="spoa's engine->Align(query, graph, &score) after the plain build loop, through the generator's own "
                                    "harness on oracle/_ref/libvcref_sisd.so (libvcref_sse41.so compared: simd_agrees); strand: the "
                                    "comparison of src/main.cpp:287-304 without the add",
                          sequences_from="tests/golden/sample.fastq.gz (kat: reads 0-39 the group, 40-54 the queries), "
                                         "tests/golden/poa_groups.json.gz (groups, gaps); `strand`: the queries of `flips` "
                                         "reverse-complemented before the call",
                          result="[score, score_rev, reversed, pairs, [node deltas, position deltas] or the SHA-256 of the pairs] "
                                 "(tests/poa_align_ref.pack / same)", full_up_to_pairs_per_entry=FULL),
              kat=kat, groups=groups, gaps=gaps, hand=hand)
    out = os.path.join(HERE, "poa_align.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(every), "entries,", sum(len(e["plain"]) + len(e["strand"]) for e in every), "alignments,",
          sum(1 for e in every if not e["simd_agrees"]), "entries where the SIMD build differs")


if __name__ == "__main__":
    main()
