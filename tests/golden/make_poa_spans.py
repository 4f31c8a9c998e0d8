"""Generates tests/golden/poa_spans.json.gz: span-limited alignment of POA group members (vc_poa_run_spans, the spans= keyword of
vechat_amd.poa) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the reference tree lies (REF, as
in oracle/Makefile): the few lines of C++ below -- this generator's own -- are compiled against spoa's public headers and linked
to oracle/_ref/libvcref_sisd.so (spoa's scalar engines, the truth) and to libvcref_sse41.so (the SIMD build, recorded as
`simd_agrees`) in a temporary directory, and run, per entry, the literal loop

    member 0, and a member without a span:   engine->Align(seq, graph)
    a member with a span:                    sub = graph.Subgraph(begin, end, &map); engine->Align(seq, sub);
                                             sub.UpdateAlignment(map, &alignment)                      (src/window.cpp:207-213)
    with `strand` (spoa's -s, src/main.cpp:287-304) both strands against the same graph or subgraph, the better one kept
    graph.AddAlignment(alignment, seq[, quality])

then GenerateMultipleSequenceAlignment(true), GenerateConsensus(&summary, false) and the graph through the accessors that
make_poa_graph.py reads.  Nothing under oracle/ is touched.

  python tests/golden/make_poa_spans.py

Entries (every one: seqs, spans -- null or [begin, end] per member, inclusive positions on member 0 --, and per algorithm "0"
kSW, "1" kNW, "2" kOV the expected consensus, coverage, members, reversed flags (strand entries), the rows and the graph tables
(number lists as first differences, tests/poa_graph_ref.pack) in full for graphs of at most FULL path entries, and always their
counts and SHA-256 (rows_sha256 over the rows joined by newlines; digest: tests/poa_graph_ref.digest)):
  seeded  SEEDED groups: a random backbone of 60 to 400 bases and 3 to 24 members cut from mutated copies (substitutions,
          insertions, deletions; some with qualities) of sub-ranges of it, their spans the true ranges jittered by a few bases;
          about one member in five is a copy of the whole backbone without a span.  5/-4/-8 linear;
  gaps    five of them at one affine and one convex score set of poa_gaps_groups.json.gz;
  strand  five of them with every second member reverse-complemented (its quality reversed), through the -s loop;
  hand    the hand-made groups below at 5/-4/-8 linear.  `all_none` is a group of poa_groups.json.gz with no span at all: its
          consensus must be the one committed there.  `repeat` is a backbone with a diverged tandem copy and a read that spells
          the first copy but belongs to the second: it also records `plain`, the same group without spans, and under kNW the two
          must differ.
"""
import ctypes as C
import gzip
import hashlib
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

import poa_graph_ref as G  # noqa: E402
import poa_strand_ref as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SPOA = os.path.join(REF, "vendor", "spoa")
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
LINEAR = (5, -4, -8, -8, -8, -8)
FULL = 1500                            # path entries up to which rows and tables are kept in full (and for the hand-made groups)
SEEDED = 12
NONE = 0xFFFFFFFF

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

// out: the graph as make_poa_graph.py's harness writes it -- nodes, per node (base, out-degree, (head, weight) ..., aligned
// nodes, their ids ...), ranks, their ids, sequences, per sequence (length, ids ...), consensus nodes, their ids --, then per
// member (reversed, score, score_rev), then rows, row size, the rows' bytes, then the coverage of every consensus base.
// Returns the count; -1: the reference threw; -2: out is too small
extern "C" int64_t spans_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals,
                             const uint32_t* sb, const uint32_t* se, int type, int m, int n, int g, int e, int q, int c,
                             int ambiguous, int64_t* out, int64_t cap) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        std::vector<std::unique_ptr<biosoup::Sequence>> sequences;
        for (uint32_t i = 0; i < k; ++i) {
            sequences.emplace_back(new biosoup::Sequence("s", 1, seqs[i], lens[i]));
            if (quals[i]) sequences.back()->quality.assign(quals[i], lens[i]);
        }
        spoa::Graph graph{};
        std::vector<int64_t> choice;
        for (uint32_t i = 0; i < k; ++i) {
            auto& it = sequences[i];
            const bool span = i != 0 && sb[i] != 0xFFFFFFFFu;
            std::vector<const spoa::Graph::Node*> map;
            spoa::Graph sub{};
            if (span) sub = graph.Subgraph(sb[i], se[i], &map);
            const spoa::Graph& target = span ? sub : graph;
            std::int32_t score = 0, score_rev = 0;
            auto alignment = engine->Align(it->data, target, &score);
            int64_t reversed = 0;
            if (ambiguous) {
                it->ReverseAndComplement();
                auto alignment_rev = engine->Align(it->data, target, &score_rev);
                if (score >= score_rev) {
                    it->ReverseAndComplement();
                } else {
                    alignment = alignment_rev;
                    reversed = 1;
                }
            }
            if (span) sub.UpdateAlignment(map, &alignment);
            if (it->quality.empty()) graph.AddAlignment(alignment, it->data);
            else graph.AddAlignment(alignment, it->data, it->quality);
            choice.push_back(reversed); choice.push_back(score); choice.push_back(score_rev);
        }
        const std::vector<std::string> msa = graph.GenerateMultipleSequenceAlignment(true);
        std::vector<uint32_t> summary;
        const std::string consensus = graph.GenerateConsensus(&summary, false);
        std::vector<int64_t> v;
        v.push_back(graph.nodes().size());
        for (const auto& it : graph.nodes()) {
            v.push_back(graph.decoder(it->code));
            v.push_back(it->outedges.size());
            for (const auto& jt : it->outedges) { v.push_back(jt->head->id); v.push_back(jt->weight); }
            v.push_back(it->aligned_nodes.size());
            for (const auto& jt : it->aligned_nodes) v.push_back(jt->id);
        }
        v.push_back(graph.rank_to_node().size());
        for (const auto& it : graph.rank_to_node()) v.push_back(it->id);
        v.push_back(graph.sequences().size());
        for (std::uint32_t i = 0; i < graph.sequences().size(); ++i) {
            std::vector<int64_t> path;
            for (auto curr = graph.sequences()[i]; curr; curr = curr->Successor(i)) path.push_back(curr->id);
            v.push_back(path.size());
            v.insert(v.end(), path.begin(), path.end());
        }
        v.push_back(graph.consensus().size());
        for (const auto& it : graph.consensus()) v.push_back(it->id);
        v.insert(v.end(), choice.begin(), choice.end());
        v.push_back(msa.size());
        v.push_back(msa.empty() ? 0 : msa[0].size());
        for (const auto& row : msa) {
            if (row.size() != msa[0].size()) return -3;
            for (const char ch : row) v.push_back(static_cast<unsigned char>(ch));
        }
        if (summary.size() != consensus.size()) return -4;
        for (const auto x : summary) v.push_back(x);
        if ((int64_t)v.size() > cap) return -2;
        for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
        return v.size();
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_harness(tmp):
    src = os.path.join(tmp, "spans_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    inc = [x for d in ("include", "src", "vendor/cereal/include", "vendor/bioparser/include", "vendor/bioparser/vendor/biosoup/include")
           for x in ("-I", os.path.join(SPOA, d))]
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"spans_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, src, "-o", out, so, "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].spans_run.restype = C.c_int64
    return libs


def run(lib, members, spans, atype, scores, ambiguous):
    """members [(bytes, bytes | None)], spans [None | (begin, end)] -> dict(tables, reversed, score, score_rev, rows, coverage)"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    UA = C.c_uint32 * max(k, 1)
    total = sum(len(s) for s, _ in members)
    cap = 64 + 16 * total + 8 * k + (k + 1) * (total + 1) + total
    out = (C.c_int64 * cap)()
    sb = UA(*[NONE if x is None else x[0] for x in spans])
    se = UA(*[NONE if x is None else x[1] for x in spans])
    n = lib.spans_run(C.c_uint32(k), SA(*[s for s, _ in members]), UA(*[len(s) for s, _ in members]), SA(*[q for _, q in members]),
                      sb, se, C.c_int(atype), *[C.c_int(x) for x in scores], C.c_int(1 if ambiguous else 0), out, C.c_int64(cap))
    assert n >= 0, n
    v, at = list(out[:n]), 0

    def take(cnt=1):
        nonlocal at
        at += cnt
        return v[at - cnt:at]
    N = take()[0]
    base, out_off, head, weight, aligned = [], [0], [], [], []
    for a in range(N):
        base.append(take()[0])
        for _ in range(take()[0]):
            h, w = take(2)
            head.append(h); weight.append(w)
        out_off.append(len(head))
        aligned += [[a, b] for b in take(take()[0]) if b > a]
    rank = take(take()[0])
    paths = [take(take()[0]) for _ in range(take()[0])]
    cons = take(take()[0])
    choice = [take(3) for _ in range(k)]
    n_rows, row_size = take(2)
    rows = [bytes(take(row_size)) for _ in range(n_rows)]
    cov = take(len(cons))
    assert at == n
    nonempty = [i for i, (s, _) in enumerate(members) if len(s)]
    assert len(paths) == len(nonempty) and n_rows == len(nonempty) + 1
    pos = [-1] * N
    for i, x in enumerate(cons):
        pos[x] = i
    rev = [c[0] for c in choice]
    tables = dict(node_base=bytes(base).decode("latin-1"), node_cons_pos=pos, rank_to_node=rank, out_off=out_off, edge_head=head,
                  edge_weight=weight, aligned=aligned, paths=[[i, rev[i], p] for i, p in zip(nonempty, paths)], cons_node=cons,
                  consensus=bytes(base[x] for x in cons).decode("latin-1"))
    return dict(tables=tables, reversed=rev, score=[c[1] for c in choice], score_rev=[c[2] for c in choice], rows=rows,
                members=nonempty, coverage=cov)


def rows_digest(rows):
    return hashlib.sha256(b"\n".join(rows)).hexdigest()


def expected(libs, members, spans, atype, scores, strand=False, full=False):
    a = run(libs["sisd"], members, spans, atype, scores, strand)
    simd = run(libs["sse41"], members, spans, atype, scores, strand)
    t = a["tables"]
    for mb, rev, path in t["paths"]:                       # every path spells the bytes that were kept
        kept = S.kept_view(members[mb][0], members[mb][1], rev)[0] if strand else members[mb][0]
        assert "".join(t["node_base"][v] for v in path).encode("latin-1") == kept, (mb, rev)
    for r, mb in zip(a["rows"], a["members"]):
        kept = S.kept_view(members[mb][0], members[mb][1], a["reversed"][mb])[0] if strand else members[mb][0]
        assert r.replace(b"-", b"") == kept
    assert a["rows"][-1].replace(b"-", b"").decode("latin-1") == t["consensus"]
    e = dict(consensus=t["consensus"], coverage=a["coverage"], members=a["members"], counts=G.counts(t), digest=G.digest(t),
             n_rows=len(a["rows"]), row_size=len(a["rows"][0]) if a["rows"] else 0, rows_sha256=rows_digest(a["rows"]),
             simd_agrees=(simd["tables"], simd["rows"], simd["coverage"]) == (t, a["rows"], a["coverage"]))
    if strand:
        e.update(reversed=a["reversed"], score=a["score"], score_rev=a["score_rev"])
    if full or e["counts"][4] <= FULL:
        e["rows"] = [r.decode("latin-1") for r in a["rows"]]
        e["tables"] = G.pack(t)
        assert G.unpack(e["tables"]) == t
    return e


# ------------------------------------------------------------------ the groups
def mutate(rng, s, rate):
    out = []
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(rng.choice("ACGT".replace(ch, "")))
            continue
        out.append(ch)
        if x < rate:
            out.append(rng.choice("ACGT"))
    return "".join(out)


def seeded_group(rng, k):
    """-> (name, [(sequence, quality or None)], [None | (begin, end)])"""
    L = (60, 97, 128, 150, 200, 256, 300, 333, 400, 64, 180, 385)[k]
    n = (3, 5, 8, 12, 17, 24, 6, 10, 24, 4, 15, 9)[k]
    rate = (0.04, 0.08, 0.12)[k % 3]
    backbone = "".join(rng.choice("ACGT") for _ in range(L))
    qual = lambda s: "".join(chr(33 + rng.randrange(3, 45)) for _ in s)   # noqa: E731
    members = [(backbone, qual(backbone) if k % 4 == 1 else None)]
    spans = [None]
    while len(members) < n:
        if rng.random() < 0.2:
            b, e, sp = 0, L - 1, None
        else:
            length = rng.randrange(max(12, L // 8), max(13, (2 * L) // 3))
            b = rng.randrange(0, L - length + 1)
            e = b + length - 1
            jb, je = min(max(b + rng.randrange(-4, 5), 0), L - 1), min(max(e + rng.randrange(-4, 5), 0), L - 1)
            sp = (min(jb, je), max(jb, je))
        s = mutate(rng, backbone[b:e + 1], rate) or backbone[b:e + 1]
        members.append((s, qual(s) if rng.random() < 0.35 else None))
        spans.append(sp)
    return f"seed{k:02d}_len{L}_n{n}", members, spans


def hand_groups(plain_fx):
    rng = random.Random(20250311)
    R = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    other = lambda ch: {"A": "C", "C": "G", "G": "T", "T": "A"}[ch]       # noqa: E731
    bb = R(90)
    L = len(bb)
    g = []
    g.append(("span_of_one_node", [(bb, None), (bb[38:43], None), (bb[40], None), (other(bb[40]), None)], [None, (40, 40), (40, 40), (40, 40)]))
    g.append(("spans_at_0_and_last", [(bb, None), (bb[:15], None), (bb[L - 15:], None), (bb[0], None), (bb[L - 1], None),
                                      (mutate(rng, bb[:22], 0.1), None), (mutate(rng, bb[L - 22:], 0.1), None)],
              [None, (0, 14), (L - 15, L - 1), (0, 0), (L - 1, L - 1), (0, 21), (L - 22, L - 1)]))
    g.append(("member_longer_than_span", [(bb, None), (bb[20:60], None), (mutate(rng, bb[10:75], 0.08), None), (bb[25:55], None)],
              [None, (30, 50), (35, 45), (30, 50)]))
    g.append(("member_shorter_than_span", [(bb, None), (bb[40:50], None), (bb[44:49], None), (mutate(rng, bb[30:42], 0.1), None)],
              [None, (10, 80), (0, L - 1), (5, 85)]))
    g.append(("empty_member_with_span", [(bb, None), ("", None), (bb[5:25], None), ("", None), (bb[10:30], None)],
              [None, (5, 20), (5, 24), None, (8, 31)]))
    # earlier whole-graph members with mismatches leave aligned nodes in the range that later spans cover
    sub = lambda s, at: "".join(other(ch) if i in at else ch for i, ch in enumerate(s))   # noqa: E731
    g.append(("span_over_aligned_nodes", [(bb, None), (sub(bb, {30, 31, 45}), None), (sub(sub(bb, {30}), {31, 45, 60}), None),
                                          (sub(bb[25:65], {5, 6}), None), (sub(bb[28:50], {3}), None), (bb[40:70], None)],
              [None, None, None, (25, 64), (28, 49), (40, 69)]))
    g.append(("two_members_same_span", [(bb, None), (mutate(rng, bb[20:70], 0.1), None), (mutate(rng, bb[20:70], 0.1), None),
                                        (bb[20:70], "".join(chr(33 + rng.randrange(3, 45)) for _ in range(50)))],
              [None, (20, 69), (20, 69), (20, 69)]))
    src = next(x for x in plain_fx["groups"] if x["name"] == "size3_len100_mixed")
    g.append(("all_none", [(s, q) for s, q in src["seqs"]], [None] * len(src["seqs"])))
    # a diverged tandem repeat: copy 2 differs from copy 1 in three places; the read spells copy 1 but lies on copy 2
    u1, unit, u2 = R(25), R(40), R(25)
    copy2 = sub(unit, {7, 19, 31})
    rep = u1 + unit + copy2 + u2
    g.append(("repeat", [(rep, None), (unit, None), (unit, None)], [None, (65, 104), (65, 104)]))
    return g


def main():
    plain_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    enc = lambda mem: [(s.encode("latin-1"), None if q is None else q.encode("latin-1")) for s, q in mem]   # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_harness(tmp)
        rng = random.Random(20250310)
        groups = [seeded_group(rng, k) for k in range(SEEDED)]
        seeded, gaps, strand, hand = [], [], [], []
        for name, mem, spans in groups:
            exp = {t: expected(libs, enc(mem), spans, int(t), LINEAR) for t in ("0", "1", "2")}
            seeded.append(dict(name=name, scores=list(LINEAR), seqs=[list(x) for x in mem], spans=spans, expected=exp))
        for name, mem, spans in groups[1:11:2]:
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                exp = {t: expected(libs, enc(mem), spans, int(t), scores) for t in ("0", "1", "2")}
                gaps.append(dict(name=name, model=model, scores=list(scores), expected=exp))
        for name, mem, spans in groups[0:10:2]:
            flips = list(range(1, len(mem), 2))
            fl = [(S.reverse_complement(s), None if q is None else q[::-1]) if i in flips else (s, q) for i, (s, q) in enumerate(enc(mem))]
            exp = {t: expected(libs, fl, spans, int(t), LINEAR, strand=True) for t in ("0", "1", "2")}
            assert any(any(e["reversed"]) for e in exp.values()), name
            strand.append(dict(name=name, scores=list(LINEAR), flips=flips, expected=exp))
        for name, mem, spans in hand_groups(plain_fx):
            exp = {t: expected(libs, enc(mem), spans, int(t), LINEAR, full=True) for t in ("0", "1", "2")}
            h = dict(name=name, scores=list(LINEAR), seqs=[list(x) for x in mem], spans=spans, expected=exp)
            if name == "all_none":
                src = next(x for x in plain_fx["groups"] if x["name"] == "size3_len100_mixed")
                assert src["scores"] == [5, -4, -8]
                for t in ("0", "1", "2"):
                    assert exp[t]["consensus"] == src["expected"][t]["consensus"], "not the committed plain consensus"
            if name == "repeat":
                h["plain"] = {t: expected(libs, enc(mem), [None] * len(mem), int(t), LINEAR, full=True) for t in ("0", "1", "2")}
                assert h["plain"]["1"]["digest"] != exp["1"]["digest"], "the repeat group does not tell the span call from the plain one"
                assert h["plain"]["1"]["rows"] != exp["1"]["rows"]
            hand.append(h)
    every = [e for grp in (seeded, gaps, strand, hand) for x in grp for e in x["expected"].values()]
    assert any(sp is not None and sp[0] == sp[1] for h in hand for sp in h["spans"])
    assert sum(1 for e in every if "tables" in e) >= 40 and any("tables" not in e for e in every)
    fx = dict(params=dict(generator="tests/golden/make_poa_spans.py",
                          reference="spoa::Graph::Subgraph / UpdateAlignment / AddAlignment of oracle/_ref/libvcref_sisd.so through the "
                                    "generator's own harness (libvcref_sse41.so compared: simd_agrees)",
                          spans="null or [begin, end] per member: inclusive positions on member 0; member 0's entry is not read",
                          strand="the members of `flips` reverse-complemented, their quality reversed, before the call; spoa's -s loop",
                          lists="first differences, tests/poa_graph_ref.unpack", digest="tests/poa_graph_ref.digest of the tables",
                          rows_sha256="SHA-256 of the rows joined by newlines", full_up_to_path_entries=FULL),
              seeded=seeded, gaps=gaps, strand=strand, hand=hand)
    out = os.path.join(HERE, "poa_spans.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(every), "entries,", sum(1 for e in every if "tables" in e), "in full,",
          sum(1 for e in every if not e["simd_agrees"]), "where the SIMD build differs")


if __name__ == "__main__":
    main()
