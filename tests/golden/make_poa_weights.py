"""Generates tests/golden/poa_weights.json.gz: explicit weights and the verbose consensus summary of POA groups
(vc_poa_run_weighted) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the reference tree lies (REF,
as in oracle/Makefile): the few lines of C++ below -- this generator's own -- are compiled against spoa's public headers and
linked to oracle/_ref/libvcref_sisd.so (the scalar engines, the bar) and libvcref_sse41.so (compared: simd_agrees), and run, per
entry, spoa's loop (src/main.cpp:277-316, with or without -s) with the AddAlignment overload each member's mode selects --
AddAlignment(alignment, seq, weight), AddAlignment(alignment, seq, weights), or the quality / plain one --, then
GenerateConsensus(&summary, true) and GenerateConsensus(&summary, false).

  python tests/golden/make_poa_weights.py

The fixture holds data only.  The sequences of `kat` are the 55 reads of sample.fastq.gz, those of `groups` and `gaps` the groups
of poa_groups.json.gz, those of `strand` the same with the members of `flips` reverse-complemented; their weights are
poa_weights_ref.seeded_weights(members, seed, kind).  Only the hand-made groups carry sequences and weights.  An entry holds the
consensus, the codes, the counts (gaps last), the coverage, the number of edges and a digest of (tail, head, weight) in
PoaGraph.edges' order (the list itself where it is short), and for -s entries the strand choices.
Asserted here on the reference: (a) the code rows sum to the coverage at every position (an entry where they do not is kept and
marked rows_sum_to_coverage: false); (b) mode 1 with weight 1 and no qualities gives the plain call's graph; (c) mode 2 with
vc_weight_lut[quality] gives the quality call's graph, edge weights included.
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
import poa_gaps_ref as pg  # noqa: E402
import poa_strand_ref as S  # noqa: E402
import poa_weights_ref as W  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")

HARNESS = r"""
#include <algorithm>
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

// modes: 0 the quality overload or the plain one, 1 seq_w[i], 2 base_w at the member's offset (reversed with a kept reverse strand).
// summary: (num_codes + 1) x cons_len.  edges: (tail, head, weight) by tail id, then out-list order.  -1: the reference threw; -2: a buffer is too small
extern "C" int weighted_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, const uint8_t* modes,
                            const uint32_t* seq_w, const uint32_t* base_w, int type, int m, int n, int g, int e, int q, int c,
                            int ambiguous, uint8_t* reversed, char* cons, uint32_t cons_cap, uint32_t* cons_len, uint32_t* n_codes,
                            uint8_t* codes, uint32_t* summary, uint64_t summary_cap, uint32_t* coverage, int64_t* edges,
                            uint64_t edges_cap, uint64_t* n_edges) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        spoa::Graph graph{};
        uint64_t at = 0;
        for (uint32_t i = 0; i < k; ++i) {
            biosoup::Sequence s("s", 1, seqs[i], lens[i]);
            if (quals[i]) s.quality.assign(quals[i], lens[i]);
            std::vector<std::uint32_t> w(base_w + at, base_w + at + lens[i]);
            at += lens[i];
            std::int32_t score = 0;
            auto alignment = engine->Align(s.data, graph, &score);
            reversed[i] = 0;
            if (ambiguous) {
                s.ReverseAndComplement();
                std::int32_t score_rev = 0;
                auto alignment_rev = engine->Align(s.data, graph, &score_rev);
                if (score >= score_rev) {
                    s.ReverseAndComplement();
                } else {
                    alignment = alignment_rev;
                    reversed[i] = 1;
                    std::reverse(w.begin(), w.end());
                }
            }
            if (modes[i] == 1) graph.AddAlignment(alignment, s.data, seq_w[i]);
            else if (modes[i] == 2) graph.AddAlignment(alignment, s.data, w);
            else if (s.quality.empty()) graph.AddAlignment(alignment, s.data);
            else graph.AddAlignment(alignment, s.data, s.quality);
        }
        std::vector<uint32_t> verbose, brief;
        const std::string consensus = graph.GenerateConsensus(&verbose, true);
        const std::string again = graph.GenerateConsensus(&brief, false);
        if (again != consensus || brief.size() != consensus.size()) return -4;
        *cons_len = consensus.size();
        *n_codes = graph.num_codes();
        if (consensus.size() > cons_cap || verbose.size() > summary_cap) return -2;
        if (verbose.size() != (uint64_t)(graph.num_codes() + 1) * consensus.size()) return -5;
        std::memcpy(cons, consensus.data(), consensus.size());
        for (uint32_t i = 0; i < graph.num_codes(); ++i) codes[i] = graph.decoder(i);
        for (size_t i = 0; i < verbose.size(); ++i) summary[i] = verbose[i];
        for (size_t i = 0; i < brief.size(); ++i) coverage[i] = brief[i];
        uint64_t ne = 0;
        for (const auto& node : graph.nodes())
            for (const auto& edge : node->outedges) {
                if (ne >= edges_cap) return -2;
                edges[3 * ne] = node->id; edges[3 * ne + 1] = edge->head->id; edges[3 * ne + 2] = edge->weight;
                ++ne;
            }
        *n_edges = ne;
        return 0;
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_harness(tmp):
    src = os.path.join(tmp, "weights_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"weights_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(REF, "vendor/spoa/include"),
                               "-I", os.path.join(REF, "vendor/spoa/vendor/cereal/include"),
                               "-I", os.path.join(REF, "vendor/spoa/vendor/bioparser/vendor/biosoup/include"), src, "-o", out, so,
                               "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].weighted_run.restype = C.c_int
    return libs


def run(lib, members, weights, atype, scores, ambiguous=False):
    """members [(bytes, bytes | None)], weights one entry per member (None, int, list) -> dict, or None where the reference threw"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    sa, qa = SA(*[s for s, _ in members]), SA(*[q for _, q in members])
    la = (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members])
    total = sum(len(s) for s, _ in members)
    modes = (C.c_uint8 * max(k, 1))(*[0 if w is None else 1 if isinstance(w, int) else 2 for w in weights])
    sw = (C.c_uint32 * max(k, 1))(*[w if isinstance(w, int) else 0 for w in weights])
    flat = [v for (s, _), w in zip(members, weights) for v in (w if isinstance(w, list) else [0] * len(s))]
    bw = (C.c_uint32 * max(total, 1))(*flat)
    cons = C.create_string_buffer(total + 1)
    rev = (C.c_uint8 * max(k, 1))()
    codes = (C.c_uint8 * 256)()
    scap, ecap = 257 * (total + 1), 2 * total + 64
    summ, cov, edges = (C.c_uint32 * scap)(), (C.c_uint32 * (total + 1))(), (C.c_int64 * (3 * ecap))()
    cons_len, n_codes, n_edges = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    rc = lib.weighted_run(C.c_uint32(k), sa, la, qa, modes, sw, bw, C.c_int(atype), *[C.c_int(x) for x in scores],
                          C.c_int(1 if ambiguous else 0), rev, cons, C.c_uint32(total + 1), C.byref(cons_len), C.byref(n_codes), codes,
                          summ, C.c_uint64(scap), cov, edges, C.c_uint64(ecap), C.byref(n_edges))
    if rc != 0:
        assert rc == -1, rc
        return None
    n, nc, ne = cons_len.value, n_codes.value, n_edges.value
    return dict(reversed=[int(x) for x in rev[:k]], consensus=cons.raw[:n], codes=bytes(codes[:nc]),
                counts=[list(summ[r * n:(r + 1) * n]) for r in range(nc + 1)], coverage=list(cov[:n]),
                edges=[tuple(edges[3 * i:3 * i + 3]) for i in range(ne)])


def entry(libs, members, weights, atype, scores, ambiguous=False):
    a = run(libs["sisd"], members, weights, atype, scores, ambiguous)
    assert a is not None
    b = run(libs["sse41"], members, weights, atype, scores, ambiguous)
    nc = len(a["codes"])
    sums = [sum(a["counts"][k][j] for k in range(nc)) for j in range(len(a["consensus"]))]
    e = dict(consensus=a["consensus"].decode("latin-1"), codes=a["codes"].decode("latin-1"), counts=a["counts"], coverage=a["coverage"],
             n_edges=len(a["edges"]), edge_digest=W.edge_digest(a["edges"]), simd_agrees=b is not None and a == b,
             rows_sum_to_coverage=sums == a["coverage"])
    if len(a["edges"]) <= 64:
        e["edges"] = [list(x) for x in a["edges"]]
    if ambiguous:
        e["reversed"] = a["reversed"]
    return e, a


def flipped(members, flips):
    fl = set(flips)
    return [(S.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(members)]


def hand_groups():
    """(name, [(sequence, quality or None)], weights): each the smallest shape at which one rule can go wrong"""
    rng = random.Random(20250519)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))     # noqa: E731
    core = rnd(24)
    x, y = core[:12] + "A" + core[12:], core[:12] + "G" + core[12:]
    g = []
    g.append(("heavy_minority", [(x, None)] * 3 + [(y, None)], [None, None, None, 10]))
    g.append(("heavy_minority_per_base", [(x, None)] * 3 + [(y, None)], [None, None, None, [10] * len(y)]))
    g.append(("zero_weight_member", [(x, None), (y, None), (y, None)], [3, 0, [0] * len(y)]))
    g.append(("zero_weight_first_member", [(x, None), (y, None)], [0, 1]))
    g.append(("uint32_wrap", [(x, None), (x, None), (y, None)], [[0x80000000] * len(x), 1, 1]))
    g.append(("uint32_wrap_mode1", [(x, None), (y, None), (y, None)], [0xFFFFFFFF, 1, 1]))
    g.append(("starts_inside_ends_early", [(core, None), (core, None), (core[6:17], None)], [None, 2, None]))
    g.append(("insertion", [(core, None), (core, None), (core[:10] + "TTT" + core[10:], None)], [None, None, 1]))
    g.append(("deletion", [(core, None), (core, None), (core[:9] + core[13:], None)], [None, None, None]))
    g.append(("three_codes_in_a_column", [(core[:12] + b + core[13:], None) for b in "AACGT"], [None] * 5))
    g.append(("code_only_off_consensus", [(core, None), (core, None), (core[:8] + "N" + core[8:], None)], [None] * 3))
    g.append(("local_finds_nothing", [("A" * 12, None), ("C" * 12, None), ("G" * 5, None)], [None, 4, [1, 2, 3, 4, 5]]))
    g.append(("empty_members", [(core, None), ("", None), (core, None), ("", None)], [None, 7, None, []]))
    g.append(("empty_members_only", [("", None), ("", None)], [3, []]))
    g.append(("empty_group", [], []))
    g.append(("group_of_one", [(core, None)], [[5] * len(core)]))
    q = lambda s: "".join(chr(33 + rng.randrange(5, 40)) for _ in s)  # noqa: E731
    g.append(("quality_beside_weights", [(lambda s: (s, q(s)))(core), (lambda s: (s, q(s)))(y), (x, None), (lambda s: (s, q(s)))(x)],
              [None, 9, None, [2] * len(x)]))
    for n in (63, 64, 65, 129):
        s = rnd(n)
        g.append((f"consensus_length_{n}", [(s, None), (s, None), (s[:n // 2] + s[n // 2 + 1:], None)], [None, 2, None]))
    s = rnd(40)
    mem = [(S_noisy(rng, s), None) for _ in range(70)]
    g.append(("seventy_members", mem, [None if i % 3 == 0 else i if i % 3 == 1 else [rng.randint(0, 9) for _ in m[0]] for i, m in enumerate(mem)]))
    return g


def S_noisy(rng, s, rate=0.06):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(rng.choice("ACGT") if r < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= r < rate:
            out.append(rng.choice("ACGT"))
    return "".join(out)


def main():
    seqs, quals = fixtures.load_sample_reads()
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    lin = lambda m, n, g: (m, n, g, g, g, g)                            # noqa: E731
    every = []
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_harness(tmp)

        def make(members, weights, t, scores, ambiguous=False):
            e, a = entry(libs, members, weights, t, scores, ambiguous)
            every.append(e)
            return e, a
        kat = []
        plain = list(zip(seqs, [None] * len(seqs)))
        for t in (0, 1, 2):
            for kind, seed in (("seq", 101), ("base", 202), ("none", 0)):
                e, _ = make(plain, W.seeded_weights(plain, seed, kind), t, lin(5, -4, -8))
                kat.append(dict(type=t, scores=[5, -4, -8], kind=kind, seed=seed, expected=e))
        # (b) and (c) on the reference, on the 55 reads and three algorithms
        withq = list(zip(seqs, quals))
        for t in (0, 1, 2):
            base = run(libs["sisd"], plain, [None] * len(plain), t, lin(5, -4, -8))
            assert base == run(libs["sisd"], plain, [1] * len(plain), t, lin(5, -4, -8)), "(b)"
            qcall = run(libs["sisd"], withq, [None] * len(withq), t, lin(5, -4, -8))
            asw = [[pg._LUT[b] for b in q] for q in quals]
            assert qcall == run(libs["sisd"], plain, asw, t, lin(5, -4, -8)), "(c)"
        groups, by_name = [], {}
        for gi, g in enumerate(poa_fx["groups"]):
            members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
            by_name[g["name"]] = members
            m, n, gp = g["scores"]
            exp = {str(t): make(members, W.seeded_weights(members, 1000 + gi, "mix"), t, lin(m, n, gp))[0] for t in (0, 1, 2)}
            groups.append(dict(name=g["name"], scores=[m, n, gp], kind="mix", seed=1000 + gi, expected=exp))
        gaps = []
        for gi, name in enumerate(GAP_GROUPS):
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                members = by_name[name]
                exp = {str(t): make(members, W.seeded_weights(members, 2000 + gi, "mix"), t, scores)[0] for t in (0, 1, 2)}
                gaps.append(dict(name=name, model=model, scores=list(scores), kind="mix", seed=2000 + gi, expected=exp))
        strand = []
        rng = random.Random(31337)
        for gi, g in enumerate(poa_fx["groups"][:10]):
            members = by_name[g["name"]]
            flips = [i for i in range(len(members)) if rng.random() < 0.5]
            fm = flipped(members, flips)
            m, n, gp = g["scores"]
            exp = {str(t): make(fm, W.seeded_weights(fm, 3000 + gi, "base"), t, lin(m, n, gp), True)[0] for t in (0, 1, 2)}
            strand.append(dict(name=g["name"], scores=[m, n, gp], flips=flips, kind="base", seed=3000 + gi, expected=exp))
        assert any(any(e["reversed"]) for s in strand for e in s["expected"].values())
        hand = []
        for name, mem, wts in hand_groups():
            members = [(s.encode(), None if q is None else q.encode()) for s, q in mem]
            exp = {str(t): make(members, wts, t, lin(5, -4, -8))[0] for t in (0, 1, 2)}
            hand.append(dict(name=name, scores=[5, -4, -8], seqs=[[s, q] for s, q in mem], weights=wts, expected=exp))
    hb = {h["name"]: h["expected"] for h in hand}
    assert hb["heavy_minority"]["1"]["consensus"][12] == "G" and hb["heavy_minority_per_base"]["1"]["consensus"][12] == "G"
    assert all(w == 4 for *_, w in hb["uint32_wrap"]["1"]["edges"][:8]), hb["uint32_wrap"]["1"]["edges"][:8]       # 2^31 + 2^31 wraps to 0, then 2 + 2
    assert any(hb["deletion"]["1"]["counts"][-1]), "no gap counted"
    assert any(not any(r) for r in hb["code_only_off_consensus"]["1"]["counts"][:-1]), "no all-zero code row"
    bad = sum(1 for e in every if not e["rows_sum_to_coverage"])
    fx = dict(params=dict(generator="tests/golden/make_poa_weights.py",
                          reference="spoa's loop (src/main.cpp:277-316) with the AddAlignment overload of every member's mode, then "
                                    "GenerateConsensus(&summary, true / false), on oracle/_ref/libvcref_sisd.so through the generator's "
                                    "own harness; libvcref_sse41.so compared (simd_agrees)",
                          sequences_from="tests/golden/sample.fastq.gz (kat, no qualities), tests/golden/poa_groups.json.gz (groups, gaps, "
                                         "strand: the members of `flips` reverse-complemented first); weights: "
                                         "poa_weights_ref.seeded_weights(members, seed, kind)",
                          asserted="(a) code rows sum to the coverage unless rows_sum_to_coverage is false; (b) weight 1 == plain; "
                                   "(c) vc_weight_lut[quality] per base == quality call"),
              kat=kat, groups=groups, gaps=gaps, strand=strand, hand=hand)
    out = os.path.join(HERE, "poa_weights.json.gz")
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(fx, separators=(",", ":")).encode())
    print(out, os.path.getsize(out), "bytes;", len(every), "entries,", bad, "where the code rows do not sum to the coverage,",
          sum(1 for e in every if not e["simd_agrees"]), "where the SIMD build differs")


if __name__ == "__main__":
    main()
