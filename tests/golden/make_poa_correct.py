"""Generates tests/golden/poa_correct.json.gz: the haplotype-aware correction of every member of a POA group (vc_poa_run_correct,
vechat_amd.poa.poa_correct) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the reference tree lies
(REF, as in oracle/Makefile).  The reference has no group form of its window flow, so the few lines of C++ below -- this
generator's own -- are the six steps of include/vechat_hip.h written with spoa's public functions (Align, AddAlignment,
GenerateConsensus, PruneGraph, LargestSubgraph, AddWeights, GenerateCorrectedSequence), compiled in a temporary directory against
spoa's public headers and linked to oracle/_ref/libvcref_sisd.so (the SIMD build libvcref_sse41.so compared: simd_agrees; the
scalar build is the bar).  Nothing built is kept.

  python tests/golden/make_poa_correct.py

Every entry has the group (`seqs`, or `group`: a name in poa_groups.json.gz), type, the six scores, the thresholds, num_prune and
`expected` (tests/poa_correct_ref.pack: consensus, scores, the corrections' lengths and the corrections, or their SHA-256 where an
entry has more than FULL bytes of them), `stats` (edges pruned, nodes lost to LargestSubgraph, edges created by AddWeights).
  groups  the 30 seeded groups of poa_groups.json.gz at local and global, their own scores, 0.22 / 0.19 / 3;
  gaps    five of them at one affine and one convex score set, local and global;
  hap     seeded two-haplotype groups: 12-24 members of 150-300 bases, two haplotypes with 3-6 SNVs and an indel between them,
          3-8 % read errors, with / without / mixed quality, each at num_prune 1, 2 and 3;
  hand    the hand-made groups below, local and global.
Asserted here, so that the fixture can fail: some entry has an edge pruned; loses nodes to LargestSubgraph; has a member whose
correction differs from its input; has two members with different corrections where the consensus is one sequence; has a
correction shorter than its member through local clipping; has an empty correction.  The count of edges that a round's
AddWeights creates is recorded and asserted to be what the engines allow: consecutive pairs that both have a node and a position
come from a diagonal step, which follows an in-edge, so the edge is always there and the count is 0 in every entry.
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

import poa_correct_ref as PC  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SPOA = os.path.join(REF, "vendor", "spoa")
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")
DEFAULTS = (0.22, 0.19, 3)             # the reference's min_confidence, min_support, num_prune
FULL = 8000                            # bytes of corrections of an entry up to which they are kept in full

HARNESS = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>
#include "spoa/spoa.hpp"

// bytes: the consensus, then every correction; meta: consensus length, per member (score, correction length), then edges pruned,
// nodes lost, edges created.  Returns the bytes written; -1: the reference threw; -2: out is too small
extern "C" int64_t correct_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, int type, int m,
                               int n, int g, int e, int q, int c, double min_confidence, double min_support, uint32_t num_prune,
                               char* out, int64_t cap, int64_t* meta) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        auto local = spoa::AlignmentEngine::Create(spoa::AlignmentType::kSW, m, n, g, e, q, c);
        spoa::Graph graph{};
        double total = 0;
        std::vector<std::string> s(k), ql(k);
        for (uint32_t i = 0; i < k; ++i) {
            s[i].assign(seqs[i], lens[i]);
            auto alignment = engine->Align(s[i], graph);
            if (quals[i]) {
                ql[i].assign(quals[i], lens[i]);
                graph.AddAlignment(alignment, s[i], ql[i]);
                for (uint32_t b = 0; b < lens[i]; ++b) total += (1 - pow(10, (33 - ql[i][b]) / 10.0));
            } else {
                graph.AddAlignment(alignment, s[i]);
                total += lens[i];
            }
        }
        std::string bytes = graph.GenerateConsensus();
        int64_t pruned = 0, lost = 0, created = 0;
        meta[0] = bytes.size();
        uint32_t first = 0;
        while (first < k && lens[first] == 0) ++first;
        if (first == k) {
            for (uint32_t i = 0; i < k; ++i) { meta[1 + 2 * i] = 0; meta[2 + 2 * i] = 0; }
        } else {
            const uint32_t L = lens[first];
            const double avg = quals[first] ? 2.0 * total / L * 1000 : 2.0 * total / L;
            auto step = [&](spoa::Graph& gr) {
                const int64_t edges = gr.edges().size();
                gr.PruneGraph(0, min_confidence, min_support, avg);
                pruned += edges - (int64_t)gr.edges().size();
                std::unique_ptr<spoa::Graph> sub(new spoa::Graph(gr.LargestSubgraph()));
                lost += (int64_t)gr.nodes().size() - (int64_t)sub->nodes().size();
                return sub;
            };
            std::unique_ptr<spoa::Graph> cur = step(graph);
            for (uint32_t r = 0; r + 1 < num_prune; ++r) {
                for (uint32_t i = 0; i < k; ++i) {
                    auto alignment = engine->Align(s[i], *cur);
                    std::vector<std::uint32_t> weights;
                    for (uint32_t b = 0; b < lens[i]; ++b) {
                        if (!quals[i]) { weights.emplace_back(1); continue; }
                        std::uint32_t weight = (1 - pow(10, (33 - ql[i][b]) / 10.0)) * 1000;
                        weights.emplace_back(weight);
                    }
                    const int64_t edges = cur->edges().size();
                    if (!alignment.empty()) cur->AddWeights(alignment, s[i].c_str(), lens[i], weights);   // (an empty one only prints)
                    created += (int64_t)cur->edges().size() - edges;
                }
                cur = step(*cur);
            }
            for (uint32_t i = 0; i < k; ++i) {
                std::int32_t score = 0;
                auto alignment = local->Align(s[i], *cur, &score);
                const std::string corr = cur->GenerateCorrectedSequence(alignment);
                meta[1 + 2 * i] = score; meta[2 + 2 * i] = corr.size();
                bytes += corr;
            }
        }
        meta[1 + 2 * k] = pruned; meta[2 + 2 * k] = lost; meta[3 + 2 * k] = created;
        if ((int64_t)bytes.size() > cap) return -2;
        std::memcpy(out, bytes.data(), bytes.size());
        return bytes.size();
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_reference(tmp):
    src = os.path.join(tmp, "correct_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    inc = [x for d in ("include", "src", "vendor/cereal/include", "vendor/bioparser/include", "vendor/bioparser/vendor/biosoup/include")
           for x in ("-I", os.path.join(SPOA, d))]
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"correct_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, src, "-o", out, so, "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].correct_run.restype = C.c_int64
    return libs


def run(lib, members, atype, scores, conf, sup, num_prune):
    """-> correct_group()-shaped dict from the reference"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    cap = 64 + 3 * sum(len(s) for s, _ in members)
    out, meta = C.create_string_buffer(cap), (C.c_int64 * (2 * k + 4))()
    n = lib.correct_run(C.c_uint32(k), SA(*[s for s, _ in members]), (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members]),
                        SA(*[q for _, q in members]), C.c_int(atype), *[C.c_int(x) for x in scores], C.c_double(conf), C.c_double(sup),
                        C.c_uint32(num_prune), out, C.c_int64(cap), meta)
    assert n >= 0, n
    raw, at = out.raw[:n], meta[0]
    reads = []
    for i in range(k):
        reads.append(raw[at:at + meta[2 + 2 * i]])
        at += meta[2 + 2 * i]
    assert at == n
    return dict(consensus=raw[:meta[0]], reads=reads, scores=[meta[1 + 2 * i] for i in range(k)],
                stats=dict(pruned=meta[1 + 2 * k], lost=meta[2 + 2 * k], created=meta[3 + 2 * k]))


CHECK = []                             # (members, result) of every entry, for the assertions at the end


def entry(libs, members, atype, scores, prune=DEFAULTS, **tags):
    r = run(libs["sisd"], members, atype, scores, *prune)
    simd = run(libs["sse41"], members, atype, scores, *prune)
    CHECK.append((members, r))
    full = sum(len(x) for x in r["reads"]) <= FULL
    return dict(type=atype, scores=list(scores), min_confidence=prune[0], min_support=prune[1], num_prune=prune[2],
                expected=PC.pack(r, full), stats=r["stats"], simd_agrees=simd == r, **tags)


def read_of(rng, hap, rate):
    out = bytearray()
    for ch in hap:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= x < rate:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def hap_group(rng, quality):
    """two haplotypes, 3-6 SNVs and an indel apart; members drawn from either with 3-8 % errors"""
    L = rng.randint(150, 300)
    h0 = bytearray(rng.choice(b"ACGT") for _ in range(L))
    h1 = bytearray(h0)
    for p in rng.sample(range(10, L - 10), rng.randint(3, 6)):
        h1[p] = rng.choice([b for b in b"ACGT" if b != h0[p]])
    p = rng.randint(20, L - 20)
    if rng.random() < 0.5:
        del h1[p:p + rng.randint(1, 3)]
    else:
        h1[p:p] = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3)))
    members = []
    for i in range(rng.randint(12, 24)):
        s = read_of(rng, h1 if i % 2 else h0, rng.uniform(0.03, 0.08))
        q = quality == "with" or (quality == "mixed" and rng.random() < 0.5)
        members.append((s, bytes(rng.randint(35, 73) for _ in s) if q else None))
    return members


def hand_groups():
    rng = random.Random(20250407)
    R = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))            # noqa: E731
    base = R(90)
    fam = [(base, None)] + [(read_of(rng, base, 0.05), None) for _ in range(5)]
    a, b = R(70), R(70)
    return [
        ("empty_member_first", [(b"", None)] + fam),
        ("empty_members_only", [(b"", None), (b"", None), (b"", None)]),
        # bytes the family does not hold: their own chain under a local build, pruned away, and then an empty local alignment
        ("unrelated_member", fam[:4] + [(b"N" * 12, None)] + fam[4:]),
        ("one_member", [(base, None)]),
        ("length_1", [(b"A", None), (b"A", None), (b"C", None)]),
        # two unrelated families: a local build leaves two components, and LargestSubgraph keeps one of them
        ("two_components", [(a, None), (b, None), (read_of(rng, a, 0.04), None), (read_of(rng, b, 0.04), None), (a, None), (b, None), (b, None)]),
    ]


def enc(members):
    return [[s.decode("latin-1"), None if q is None else q.decode("latin-1")] for s, q in members]


def main():
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_reference(tmp)
        by_name = {}
        for g in poa_fx["groups"]:
            members = [(s.encode("latin-1"), None if q is None else q.encode("latin-1")) for s, q in g["seqs"]]
            by_name[g["name"]] = members
            m, n, gp = g["scores"]
            for t in (0, 1):
                entries.append(entry(libs, members, t, (m, n, gp, gp, gp, gp), kind="groups", group=g["name"]))
        for name in GAP_GROUPS:
            for model, key in GAP_SETS.items():
                for t in (0, 1):
                    entries.append(entry(libs, by_name[name], t, tuple(gaps_fx["scores"][key]), kind="gaps", group=name, model=model))
        rng = random.Random(20250408)
        for i, quality in enumerate(("with", "without", "mixed", "with", "without", "mixed")):
            members = hap_group(rng, quality)
            scores = (5, -4, -8, -8, -8, -8) if i < 3 else (5, -4, -8, -6, -8, -6) if i == 3 else (3, -5, -4, -4, -4, -4)
            for k in (1, 2, 3):
                entries.append(entry(libs, members, 1 if i != 4 else 0, scores, (0.22, 0.19, k), kind="hap", name=f"hap{i}_{quality}",
                                     seqs=enc(members)))
        for name, members in hand_groups():
            for t in (0, 1):
                entries.append(entry(libs, members, t, (5, -4, -8, -8, -8, -8), kind="hand", name=name, seqs=enc(members)))

    # the fixture can fail
    assert any(r["stats"]["pruned"] for _, r in CHECK), "no edge pruned"
    assert any(r["stats"]["lost"] for _, r in CHECK), "no node lost to LargestSubgraph"
    assert all(r["stats"]["created"] == 0 for _, r in CHECK), "AddWeights created an edge: the docstring's argument is wrong"
    assert any(x != s for ms, r in CHECK for (s, _), x in zip(ms, r["reads"]) if x), "no correction differs from its input"
    assert any(len({x for x in r["reads"] if len(x) > 100}) > 1 for _, r in CHECK), "no entry with two different corrections"
    assert any(0 < len(x) < len(s) and x in s for ms, r in CHECK for (s, _), x in zip(ms, r["reads"])), "no correction clipped by the local engine"
    assert any(s and not x for ms, r in CHECK for (s, _), x in zip(ms, r["reads"])), "no empty correction of a non-empty member"
    fx = dict(params=dict(generator="tests/golden/make_poa_correct.py",
                          reference="the six steps of vc_poa_run_correct (include/vechat_hip.h) written with spoa's Align, AddAlignment, "
                                    "GenerateConsensus, PruneGraph, LargestSubgraph, AddWeights and GenerateCorrectedSequence, through the "
                                    "generator's own harness on oracle/_ref/libvcref_sisd.so (libvcref_sse41.so compared: simd_agrees)",
                          sequences_from="tests/golden/poa_groups.json.gz (`group`), or the entry's own `seqs`",
                          result="tests/poa_correct_ref.pack / same", full_up_to_bytes_per_entry=FULL),
              entries=entries)
    out = os.path.join(HERE, "poa_correct.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(entries), "entries,", sum(len(r["reads"]) for _, r in CHECK), "corrections,",
          sum(1 for e in entries if not e["simd_agrees"]), "entries where the SIMD build differs;",
          "pruned", sum(r["stats"]["pruned"] for _, r in CHECK), "lost", sum(r["stats"]["lost"] for _, r in CHECK),
          "created", sum(r["stats"]["created"] for _, r in CHECK))


if __name__ == "__main__":
    main()
