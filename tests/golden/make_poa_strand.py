"""Generates tests/golden/poa_strand.json.gz: strand-ambiguous POA groups (vc_poa_run_strand, spoa's `-s`) from the REAL
reference.  Runs where oracle/_ref was built (after build()) and the reference tree lies (REF, as in oracle/Makefile): the few
lines of C++ below -- this generator's own -- are compiled against spoa's public headers and biosoup's sequence.hpp and linked
to oracle/_ref/libvcref_sisd.so (spoa's scalar engines) and to libvcref_sse41.so (the SIMD build) in a temporary directory, and
run, per entry, the loop of spoa's command line (src/main.cpp:277-316): Align, ReverseAndComplement, Align, the choice,
AddAlignment; then GenerateMultipleSequenceAlignment(true) and GenerateConsensus(&summary, false).

  python tests/golden/make_poa_strand.py

The fixture holds flip lists and results only.  The sequences of `kat` are the 55 reads of sample.fastq.gz and those of `groups`
and `gaps` the groups of poa_groups.json.gz; the members named in `flips` are reverse-complemented (with the quality string
reversed) before the call -- by the test, with tests/poa_strand_ref.reverse_complement.  Only the hand-made groups carry their
sequences.
  kat     every entry of spoa_kat_gaps.json (three algorithms x linear / affine / convex, with and without qualities), every
          second read flipped;
  groups  the 30 seeded groups, a seeded flip list each (every third list flips member 0, so that the consensus comes out on
          the other strand and reversed == flip XOR flip[0] is exercised), all three algorithms at the group's scores;
  gaps    five of those groups at one affine and one convex score set, as GAP_GROUPS of make_poa_msa.py;
  hand    lower-case, U and lower-case IUPAC members kept and reversed (the round trip), a reverse-palindromic member (the tie
          keeps forward), local alignments that find nothing on either strand / only in reverse, empty members between others, a
          single member, an empty group.
Every entry is the SCALAR build's; where the SIMD build differs `simd_agrees: false` records it.  Asserted here, so that the
fixture cannot prove nothing: at least half of the entries have a reversed member; one has an exact tie score == score_rev != 0;
one has a kept forward member whose bytes change in the round trip; and for every entry without such a member the reference's
PLAIN loop (the flow of the existing fixtures) on the kept views gives the same consensus, rows and coverage.  With such a member
it need not: spoa aligned it on its bytes as given and added the round-tripped ones, while the plain loop aligns the latter;
`plain_agrees` records what was seen there.
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
import poa_strand_ref as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
TYPES = {"SW": 0, "NW": 1, "OV": 2}
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")

HARNESS = r"""
#include <atomic>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>
#include "biosoup/sequence.hpp"
#include "spoa/spoa.hpp"

std::atomic<std::uint32_t> biosoup::Sequence::num_objects{0};

// ambiguous: the command line's loop with -s; otherwise its plain loop.  kept / kept_q: the members as they were added, back to
// back.  rows: n_rows x row_size bytes.  -1: the reference threw; -2: a buffer is too small
extern "C" int strand_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, int type,
                          int m, int n, int g, int e, int q, int c, int ambiguous, uint8_t* reversed, int32_t* score_fwd,
                          int32_t* score_rc, char* kept, char* kept_q, char* rows, uint64_t rows_cap, uint32_t* n_rows,
                          uint32_t* row_size, char* cons, uint32_t cons_cap, uint32_t* cons_len, uint32_t* coverage) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        std::vector<std::unique_ptr<biosoup::Sequence>> sequences;
        for (uint32_t i = 0; i < k; ++i) {
            sequences.emplace_back(new biosoup::Sequence("s", 1, seqs[i], lens[i]));
            if (quals[i]) sequences.back()->quality.assign(quals[i], lens[i]);
        }
        spoa::Graph graph{};
        uint32_t at = 0, idx = 0;
        for (const auto& it : sequences) {
            std::int32_t score = 0;
            auto alignment = engine->Align(it->data, graph, &score);
            reversed[idx] = 0; score_fwd[idx] = score; score_rc[idx] = 0;
            if (ambiguous) {
                it->ReverseAndComplement();
                std::int32_t score_rev = 0;
                auto alignment_rev = engine->Align(it->data, graph, &score_rev);
                score_rc[idx] = score_rev;
                if (score >= score_rev) {
                    it->ReverseAndComplement();
                } else {
                    alignment = alignment_rev;
                    reversed[idx] = 1;
                }
            }
            if (it->quality.empty()) graph.AddAlignment(alignment, it->data);
            else graph.AddAlignment(alignment, it->data, it->quality);
            std::memcpy(kept + at, it->data.data(), it->data.size());
            if (!it->quality.empty()) std::memcpy(kept_q + at, it->quality.data(), it->quality.size());
            at += it->data.size();
            ++idx;
        }
        const std::vector<std::string> msa = graph.GenerateMultipleSequenceAlignment(true);
        std::vector<uint32_t> summary;
        const std::string consensus = graph.GenerateConsensus(&summary, false);
        *n_rows = msa.size();
        *row_size = msa.empty() ? 0 : msa[0].size();
        *cons_len = consensus.size();
        if ((uint64_t)msa.size() * *row_size > rows_cap || consensus.size() > cons_cap) return -2;
        for (size_t i = 0; i < msa.size(); ++i) {
            if (msa[i].size() != *row_size) return -3;
            std::memcpy(rows + i * (uint64_t)*row_size, msa[i].data(), *row_size);
        }
        std::memcpy(cons, consensus.data(), consensus.size());
        if (summary.size() != consensus.size()) return -4;
        for (size_t i = 0; i < summary.size(); ++i) coverage[i] = summary[i];
        return 0;
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_harness(tmp):
    """-> {"sisd": CDLL, "sse41": CDLL}: the harness linked to each build of the reference"""
    src = os.path.join(tmp, "strand_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"strand_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(REF, "vendor/spoa/include"),
                               "-I", os.path.join(REF, "vendor/spoa/vendor/cereal/include"),
                               "-I", os.path.join(REF, "vendor/spoa/vendor/bioparser/vendor/biosoup/include"), src, "-o", out, so,
                               "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].strand_run.restype = C.c_int
    return libs


def run(lib, members, atype, scores, ambiguous):
    """members [(bytes, bytes | None)] -> dict, or None where the reference threw"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    sa = SA(*[s for s, _ in members])
    qa = SA(*[q for _, q in members])
    la = (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members])
    total = sum(len(s) for s, _ in members)
    cap = (k + 1) * (total + 1)
    rows = C.create_string_buffer(max(cap, 1))
    cons, kept, kept_q = (C.create_string_buffer(total + 1) for _ in range(3))
    cov = (C.c_uint32 * (total + 1))()
    rev = (C.c_uint8 * max(k, 1))()
    sc, scr = (C.c_int32 * max(k, 1))(), (C.c_int32 * max(k, 1))()
    n_rows, row_size, cons_len = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib.strand_run(C.c_uint32(k), sa, la, qa, C.c_int(atype), *[C.c_int(x) for x in scores], C.c_int(1 if ambiguous else 0),
                        rev, sc, scr, kept, kept_q, rows, C.c_uint64(cap), C.byref(n_rows), C.byref(row_size), cons,
                        C.c_uint32(total + 1), C.byref(cons_len), cov)
    if rc != 0:
        return None
    rs = row_size.value
    views, at = [], 0
    for s, q in members:
        views.append((kept.raw[at:at + len(s)], None if q is None else kept_q.raw[at:at + len(s)]))
        at += len(s)
    return dict(reversed=[int(x) for x in rev[:k]], score=list(sc[:k]), score_rev=list(scr[:k]), kept=views,
                rows=[rows.raw[i * rs:(i + 1) * rs] for i in range(n_rows.value)], consensus=cons.raw[:cons_len.value],
                coverage=list(cov[:cons_len.value]))


def flipped(members, flips):
    fl = set(flips)
    return [(S.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(members)]


def entry(libs, members, atype, scores):
    """one fixture entry from the scalar build: the strand flow, compared with the SIMD build and with the plain flow on the
    kept views"""
    a = run(libs["sisd"], members, atype, scores, True)
    assert a is not None
    b = run(libs["sse41"], members, atype, scores, True)
    simd_agrees = b is not None and all(a[k] == b[k] for k in a)
    for (s, q), (ks, kq), r in zip(members, a["kept"], a["reversed"]):
        assert (ks, kq) == S.kept_view(s, q, r)
    # the existing fixtures' flow on the kept views.  It must give the same graph -- unless the round trip changed a kept forward
    # member: spoa aligned that one on its bytes as given (a `u` or a lower-case letter matches no node) and the plain flow
    # aligns the round-tripped ones, so the two may differ by construction; there plain_agrees only records what was seen.
    changed = any(not r and ks != s for (s, _), (ks, _), r in zip(members, a["kept"], a["reversed"]))
    plain = run(libs["sisd"], a["kept"], atype, scores, False)
    assert plain is not None
    plain_agrees = (plain["consensus"], plain["rows"], plain["coverage"]) == (a["consensus"], a["rows"], a["coverage"])
    assert plain_agrees or changed
    nonempty = [i for i, (s, _) in enumerate(members) if len(s)]
    assert len(a["rows"]) == len(nonempty) + 1
    for r, i in zip(a["rows"], nonempty):
        assert r.replace(b"-", b"") == a["kept"][i][0]
    return dict(reversed=a["reversed"], score=a["score"], score_rev=a["score_rev"], rows=[r.decode() for r in a["rows"]],
                members=nonempty, consensus=a["consensus"].decode(), coverage=a["coverage"], simd_agrees=simd_agrees,
                round_trip_changes=changed, plain_agrees=plain_agrees)


def noisy(rng, s, rate=0.06):
    """a copy with deletions, substitutions and insertions, a third of `rate` each"""
    out = []
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
            continue
        out.append(ch)
        if x < rate:
            out.append(rng.choice("ACGT"))
    return "".join(out)


def hand_groups():
    rng = random.Random(20240611)
    base = "".join(rng.choice("ACGT") for _ in range(90))
    rc = lambda s: S.reverse_complement(s.encode()).decode()              # noqa: E731

    def dress(s, letters):
        """a few bases replaced by lower-case letters, U and IUPAC codes"""
        s = list(s)
        for k, ch in zip(range(5, len(s), max(1, len(s) // (len(letters) + 1))), letters):
            s[k] = ch if ch in "uUrykmswnbdhvRYKMSWN" else s[k].lower()
        return "".join(s)
    q = lambda s: "".join(chr(33 + rng.randrange(5, 40)) for _ in s)      # noqa: E731
    g = []
    g.append(("round_trip_kept_and_reversed",
              [(dress(base, "xxuU"), None), (dress(noisy(rng, base), "xrykmxu"), None), (dress(rc(noisy(rng, base)), "xxbdhvsU"), None),
               (noisy(rng, base), None), (dress(rc(noisy(rng, base)), "uswnNx"), None), (dress(noisy(rng, base), "USWNsxxU"), None)]))
    g.append(("round_trip_with_qualities",
              [(lambda s: (s, q(s)))(dress(base, "xux")), (lambda s: (s, q(s)))(dress(rc(noisy(rng, base)), "xxUr")),
               (lambda s: (s, q(s)))(dress(noisy(rng, base), "xyU")), (rc(noisy(rng, base)), None)]))
    g.append(("all_lower_case", [(base, None), (noisy(rng, base).lower(), None), (rc(noisy(rng, base)).lower(), None)]))
    g.append(("reverse_palindrome_tie", [("ACGT" * 10, None), ("ACGT" * 10, None), ("ACGT" * 8, None), ("ACGT" * 10, q("ACGT" * 10))]))
    g.append(("local_nothing_on_either_strand", [("A" * 12, None), ("C" * 12, None), ("ACAC", None)]))
    g.append(("local_only_in_reverse", [("A" * 14, None), ("T" * 14, None), ("TTTTTTCTTTTT", None), ("AAAAAAGAAAAAAA", None)]))
    g.append(("empty_members_between", [(base, None), ("", None), (lambda s: (s, q(s)))(rc(noisy(rng, base))), ("", None),
                                        (noisy(rng, base), None), ("", None)]))
    g.append(("empty_member_first", [("", None), (rc(base), None), (noisy(rng, base), None)]))
    g.append(("single_member", [(dress(base, "xuU"), None)]))
    g.append(("single_member_reverse_palindrome", [("ACGT" * 5, None)]))
    g.append(("empty_members_only", [("", None), ("", None)]))
    g.append(("empty_group", []))
    return g


def main():
    seqs, quals = fixtures.load_sample_reads()
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    rng = random.Random(977)
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_harness(tmp)
        kat = {}
        kat_flips = list(range(1, len(seqs), 2))
        for name, k in json.load(open(os.path.join(HERE, "spoa_kat_gaps.json"))).items():
            members = flipped(list(zip(seqs, quals if k["quality"] else [None] * len(seqs))), kat_flips)
            scores = (k["m"], k["n"], k["g"], k["e"], k["q"], k["c"])
            kat[name] = dict(type=k["type"], scores=list(scores), quality=k["quality"], flips=kat_flips,
                             **entry(libs, members, TYPES[k["type"]], scores))
        groups, by_name, flips_of = [], {}, {}
        for gi, g in enumerate(poa_fx["groups"]):
            members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
            flips = [i for i in range(len(members)) if rng.random() < 0.5]
            if gi % 3 == 0 and members and 0 not in flips:
                flips = [0] + flips
            by_name[g["name"]], flips_of[g["name"]] = members, flips
            m, n, gp = g["scores"]
            exp = {t: entry(libs, flipped(members, flips), int(t), (m, n, gp, gp, gp, gp)) for t in ("0", "1", "2")}
            groups.append(dict(name=g["name"], scores=[m, n, gp], flips=flips, expected=exp))
        gaps = []
        for name in GAP_GROUPS:
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                exp = {t: entry(libs, flipped(by_name[name], flips_of[name]), int(t), scores) for t in ("0", "1", "2")}
                gaps.append(dict(name=name, model=model, scores=list(scores), flips=flips_of[name], expected=exp))
        hand = []
        for name, mem in hand_groups():
            members = [(s.encode(), None if q is None else q.encode()) for s, q in mem]
            exp = {t: entry(libs, members, int(t), (5, -4, -8, -8, -8, -8)) for t in ("0", "1", "2")}
            hand.append(dict(name=name, scores=[5, -4, -8], seqs=[[s, q] for s, q in mem], expected=exp))
            if name.startswith("round_trip"):
                sc = (5, -4, -8, -6, -10, -4)
                exp = {t: entry(libs, members, int(t), sc) for t in ("0", "1", "2")}
                hand.append(dict(name=name + "_convex", scores=list(sc), seqs=[[s, q] for s, q in mem], expected=exp))
    every = list(kat.values()) + [g["expected"][t] for g in groups + gaps + hand for t in ("0", "1", "2")]
    with_rev = sum(1 for e in every if any(e["reversed"]))
    assert 2 * with_rev >= len(every), (with_rev, len(every))
    assert any(a == b != 0 for e in every for a, b in zip(e["score"], e["score_rev"])), "no exact tie with a non-zero score"
    assert any(e["round_trip_changes"] for e in every), "no kept member changes in the round trip"
    hb = {g["name"]: g["expected"] for g in hand}
    assert not any(hb["reverse_palindrome_tie"]["1"]["reversed"])
    assert hb["local_nothing_on_either_strand"]["0"]["score"][:2] == [0, 0] == hb["local_nothing_on_either_strand"]["0"]["score_rev"][:2]
    assert hb["local_only_in_reverse"]["0"]["reversed"][1] == 1 and hb["local_only_in_reverse"]["0"]["score"][1] == 0
    fx = dict(params=dict(generator="tests/golden/make_poa_strand.py",
                          reference="the loop of spoa's src/main.cpp:277-316 on oracle/_ref/libvcref_sisd.so through the "
                                    "generator's own harness; libvcref_sse41.so compared (simd_agrees)",
                          sequences_from="tests/golden/sample.fastq.gz (kat), tests/golden/poa_groups.json.gz (groups, gaps); the "
                                         "members of `flips` are reverse-complemented, with their quality reversed, before the call"),
              kat=kat, groups=groups, gaps=gaps, hand=hand)
    out = os.path.join(HERE, "poa_strand.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(every), "entries,", with_rev, "with a reversed member,",
          sum(1 for e in every if not e["simd_agrees"]), "where the SIMD build differs")


if __name__ == "__main__":
    main()
