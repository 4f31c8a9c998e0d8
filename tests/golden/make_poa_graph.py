"""Generates tests/golden/poa_graph.json.gz: the partial order graph of POA groups (vc_poa_run_graph, vechat_amd.poa.poa_graph,
PoaGraph.to_gfa / to_dot) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the reference tree lies
(REF, as in oracle/Makefile).  Two sources of truth, both built in a temporary directory, nothing of them kept:

  arrays  the few lines of C++ below -- this generator's own -- compiled against spoa's public headers and linked to
          oracle/_ref/libvcref_sisd.so (the SIMD build libvcref_sse41.so compared: simd_agrees): the plain loop or the -s loop of
          spoa's command line (src/main.cpp:277-316), GenerateConsensus(), then the graph through its public accessors only --
          nodes(), their outedges and aligned_nodes, rank_to_node(), sequences(), Node::Successor, consensus(), decoder();
  text    spoa's own command line (src/main.cpp with graph.cpp, alignment_engine.cpp, sisd_alignment_engine.cpp, dispatcher.cpp)
          run on a temporary FASTA / FASTQ of the group with explicit -l -m -n -g -e -q -c: the stdout of -r 3, -r 4 and the file
          of -d for the group as it is, and of -r 4 -s -d for the group with its flip list applied.  Only for groups of upper-case
          bases without an empty record and without an all-'!' quality string: there spoa's reader and the project's agree and
          spoa's indexing of headers by added sequence is not in play.  A text is kept as its length and SHA-256, and in full
          where it is shorter than 3 000 bytes.

  python tests/golden/make_poa_graph.py

Entries (each: `plain`, the group as it is, and `strand`, the group with the members of `flips` reverse-complemented and their
quality reversed -- by the test, with tests/poa_strand_ref.reverse_complement -- run with -s).  Every graph has `counts` (nodes,
edges, aligned pairs, paths, path entries) and `digest`, the SHA-256 of its tables in canonical form (tests/poa_graph_ref.digest);
the tables themselves (`tables`, number lists as first differences, tests/poa_graph_ref.pack / unpack) are kept in full for the
hand-made groups, for one known answer and for every graph of at most 3 000 path entries: all 342 in full are 2 MB compressed,
ten times the bound set for this file.
  kat     every entry of spoa_kat_gaps.json on the 55 reads of sample.fastq.gz, flips as in poa_strand.json.gz; text for the
          linear ones without qualities (the first read's quality string is all '!', so the three with qualities are not text groups);
  groups  the 30 seeded groups of poa_groups.json.gz at the three algorithms, flips as in poa_strand.json.gz;
  gaps    five of them at one affine and one convex score set;
  hand    the hand-made groups below, with their sequences, and with text where the rules above allow it.
Asserted here, so that the fixture cannot prove nothing: an entry has a reversed path, one an aligned block of 3 or more nodes,
one a node of out-degree 3 or more, one weights from qualities; every path spells its kept bytes; and the arrays formatted by
PoaGraph.to_gfa / to_dot are the recorded text.
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

import fixtures  # noqa: E402
import poa_graph_ref as G  # noqa: E402
import poa_strand_ref as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SPOA = os.path.join(REF, "vendor", "spoa")
TYPES = {"SW": 0, "NW": 1, "OV": 2}
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")
FULL_TEXT = 3000
FULL_TABLES = 3000                     # path entries up to which a graph's tables are kept in full (and for FULL_KAT, the hand-made groups)
FULL_KAT = ("GlobalWithQualities",)

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

// out: nodes, per node (base, out-degree, (head, weight) ..., aligned nodes, their ids ...), ranks, their ids, sequences, per
// sequence (length, ids ...), consensus nodes, their ids, then a reversed flag per member.  Returns the count; -1: the reference
// threw; -2: out is too small
extern "C" int64_t graph_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, int type,
                             int m, int n, int g, int e, int q, int c, int ambiguous, int64_t* out, int64_t cap) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        std::vector<std::unique_ptr<biosoup::Sequence>> sequences;
        for (uint32_t i = 0; i < k; ++i) {
            sequences.emplace_back(new biosoup::Sequence("s", 1, seqs[i], lens[i]));
            if (quals[i]) sequences.back()->quality.assign(quals[i], lens[i]);
        }
        spoa::Graph graph{};
        std::vector<int64_t> reversed;
        for (const auto& it : sequences) {
            std::int32_t score = 0;
            auto alignment = engine->Align(it->data, graph, &score);
            reversed.push_back(0);
            if (ambiguous) {
                it->ReverseAndComplement();
                std::int32_t score_rev = 0;
                auto alignment_rev = engine->Align(it->data, graph, &score_rev);
                if (score >= score_rev) {
                    it->ReverseAndComplement();
                } else {
                    alignment = alignment_rev;
                    reversed.back() = 1;
                }
            }
            if (it->quality.empty()) graph.AddAlignment(alignment, it->data);
            else graph.AddAlignment(alignment, it->data, it->quality);
        }
        graph.GenerateConsensus();
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
        v.insert(v.end(), reversed.begin(), reversed.end());
        if ((int64_t)v.size() > cap) return -2;
        for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
        return v.size();
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_reference(tmp):
    """-> ({"sisd": CDLL, "sse41": CDLL}, path of spoa's command line built from its own main.cpp)"""
    src = os.path.join(tmp, "graph_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    inc = [x for d in ("include", "src", "vendor/cereal/include", "vendor/bioparser/include", "vendor/bioparser/vendor/biosoup/include")
           for x in ("-I", os.path.join(SPOA, d))]
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"graph_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, src, "-o", out, so, "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].graph_run.restype = C.c_int64
    cli = os.path.join(tmp, "spoa_cli")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", *inc, "-DSPOA_VERSION=\"x\"",
                           *[os.path.join(SPOA, "src", f) for f in ("main.cpp", "graph.cpp", "alignment_engine.cpp", "sisd_alignment_engine.cpp",
                                                                    "dispatcher.cpp")], "-o", cli, "-lz"])
    return libs, cli


def run(lib, members, atype, scores, ambiguous):
    """members [(bytes, bytes | None)] -> poa_graph_ref.tables()-shaped dict, from the reference"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    total = sum(len(s) for s, _ in members)
    cap = 64 + 16 * total + 4 * k
    out = (C.c_int64 * cap)()
    n = lib.graph_run(C.c_uint32(k), SA(*[s for s, _ in members]), (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members]),
                      SA(*[q for _, q in members]), C.c_int(atype), *[C.c_int(x) for x in scores], C.c_int(1 if ambiguous else 0), out,
                      C.c_int64(cap))
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
    rev = take(k)
    assert at == n
    nonempty = [i for i, (s, _) in enumerate(members) if len(s)]
    assert len(paths) == len(nonempty)
    pos = [-1] * N
    for i, x in enumerate(cons):
        pos[x] = i
    return dict(node_base=bytes(base).decode("latin-1"), node_cons_pos=pos, rank_to_node=rank, out_off=out_off, edge_head=head,
                edge_weight=weight, aligned=aligned, paths=[[i, rev[i], p] for i, p in zip(nonempty, paths)], cons_node=cons,
                consensus=bytes(base[x] for x in cons).decode("latin-1"))


def flipped(members, flips):
    fl = set(flips)
    return [(S.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(members)]


def text_ok(members):
    return bool(members) and all(len(s) and s == s.upper() and s.isalpha() and (q is None or set(q) != {0x21}) for s, q in members) and \
        len({q is None for _, q in members}) == 1                          # one file is FASTA or FASTQ, not both


def recorded(text):
    r = dict(bytes=len(text), sha256=hashlib.sha256(text).hexdigest())
    if len(text) < FULL_TEXT:
        r["text"] = text.decode("latin-1")
    return r


def cli_text(cli, tmp, members, names, atype, scores, strand):
    """spoa's command line on the group -> {"gfa", "gfa_consensus", "dot"} (plain) or {"gfa_consensus", "dot"} (-s), raw bytes"""
    fastq = members[0][1] is not None
    path = os.path.join(tmp, "group.fastq" if fastq else "group.fasta")
    with open(path, "wb") as f:
        for nm, (s, q) in zip(names, members):
            f.write(b"@%s\n%s\n+\n%s\n" % (nm.encode(), s, q) if fastq else b">%s\n%s\n" % (nm.encode(), s))
    m, n, g, e, q, c = scores
    common = [cli, "-l", str(atype), "-m", str(m), "-n", str(n), "-g", str(g), "-e", str(e), "-q", str(q), "-c", str(c)]
    dot = os.path.join(tmp, "group.dot")
    if os.path.exists(dot):
        os.remove(dot)
    if strand:
        out = dict(gfa_consensus=subprocess.check_output(common + ["-r", "4", "-s", "-d", dot, path]))
    else:
        out = dict(gfa=subprocess.check_output(common + ["-r", "3", path]), gfa_consensus=subprocess.check_output(common + ["-r", "4", path]))
        subprocess.check_output(common + ["-d", dot, path])
    out["dot"] = open(dot, "rb").read()
    return out


def variant(libs, cli, tmp, members, names, atype, scores, strand, want_text, full):
    a = run(libs["sisd"], members, atype, scores, strand)
    simd = run(libs["sse41"], members, atype, scores, strand)
    # every path spells the bytes that were kept
    for mb, rev, path in a["paths"]:
        kept = S.kept_view(members[mb][0], members[mb][1], rev)[0] if strand else members[mb][0]
        assert "".join(a["node_base"][v] for v in path).encode("latin-1") == kept, (mb, rev)
        assert rev == 0 or strand
    assert "".join(a["node_base"][v] for v in a["cons_node"]) == a["consensus"]
    e = dict(counts=G.counts(a), digest=G.digest(a), simd_agrees=simd == a)
    if full or e["counts"][4] <= FULL_TABLES:
        e["tables"] = G.pack(a)
        assert G.unpack(e["tables"]) == a
    CHECK.append(a)
    if want_text and text_ok(members):
        raw = cli_text(cli, tmp, members, names, atype, scores, strand)
        pg = G.to_poa_graph(a)
        if not strand:
            assert pg.to_gfa(names) == raw["gfa"], "to_gfa differs from spoa -r 3"
        assert pg.to_gfa(names, include_consensus=True) == raw["gfa_consensus"], "to_gfa differs from spoa -r 4"
        assert pg.to_dot() == raw["dot"], "to_dot differs from spoa -d"
        e["text"] = {k: recorded(t) for k, t in raw.items()}
    return e


CHECK = []                             # every graph in full, for the assertions at the end


def entry(libs, cli, tmp, members, names, atype, scores, flips, want_text, full=False):
    return dict(plain=variant(libs, cli, tmp, members, names, atype, scores, False, want_text, full),
                strand=variant(libs, cli, tmp, flipped(members, flips), names, atype, scores, True, want_text, full))


def noisy(rng, s, rate=0.06):
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
    """[(name, [(sequence, quality or None)], flips)]"""
    rng = random.Random(20250117)
    R = lambda n: "".join(rng.choice("ACGT") for _ in range(n))           # noqa: E731
    q = lambda s: "".join(chr(33 + rng.randrange(5, 40)) for _ in s)      # noqa: E731
    base = R(90)
    g = [("empty_group", [], []),
         ("empty_members_only", [("", None), ("", None)], []),
         ("empty_members_between", [("", None), (base, None), ("", None), (lambda s: (s, q(s)))(noisy(rng, base)),
                                    (noisy(rng, base), None), ("", None)], [4]),
         ("single_member", [(base, None)], [])]
    # graphs of exactly 63, 64 and 65 nodes, the tile boundary of the device's prefix sums: a chain of 60 and one read that adds
    # 3, 4 or 5 nodes (an insertion in the middle)
    chain = R(60)
    for extra in (3, 4, 5):
        ins = {"A": "C", "C": "G", "G": "T", "T": "A"}[chain[30]] * extra
        g.append((f"nodes_{60 + extra}", [(chain, None), (chain[:30] + ins + chain[30:], None), (chain, None)], [2]))
    short = R(20)
    g.append(("members_70_of_20_bases", [(noisy(rng, short, 0.1) or short, None) for _ in range(70)], list(range(1, 70, 3))))
    # one position with four different bases between equal flanks: a column of 4 mutually aligned nodes, and their common
    # predecessor has out-degree 4
    l, r = R(15), R(15)
    g.append(("out_degree_4_and_aligned_column_of_4", [(l + b + r, None) for b in "ACGTAC"], [3]))
    g.append(("weights_from_qualities", [(lambda s: (s, q(s)))(noisy(rng, base)) for _ in range(5)], [2, 3]))
    g.append(("reversed_member_0", [(noisy(rng, base), None) for _ in range(6)], [0, 2]))
    return g


def main():
    seqs, quals = fixtures.load_sample_reads()
    raw = gzip.open(os.path.join(HERE, "sample.fastq.gz"), "rt").read().split("\n")
    kat_names = [l[1:].split()[0] for l in raw[0::4] if l]
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    strand_fx = json.load(gzip.open(os.path.join(HERE, "poa_strand.json.gz"), "rt"))
    flips_of = {g["name"]: g["flips"] for g in strand_fx["groups"]}
    with tempfile.TemporaryDirectory() as tmp:
        libs, cli = build_reference(tmp)
        kat = {}
        for name, k in json.load(open(os.path.join(HERE, "spoa_kat_gaps.json"))).items():
            members = list(zip(seqs, quals if k["quality"] else [None] * len(seqs)))
            scores = (k["m"], k["n"], k["g"], k["e"], k["q"], k["c"])
            flips = strand_fx["kat"][name]["flips"]
            linear = k["g"] == k["e"]
            kat[name] = dict(type=k["type"], scores=list(scores), quality=k["quality"], flips=flips,
                             **entry(libs, cli, tmp, members, kat_names, TYPES[k["type"]], scores, flips, linear, name in FULL_KAT))
            assert CHECK[-2]["consensus"] == k["consensus"], name
        groups, by_name = [], {}
        for g in poa_fx["groups"]:
            members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
            by_name[g["name"]] = members
            m, n, gp = g["scores"]
            names = [f"r{i}" for i in range(len(members))]
            exp = {t: entry(libs, cli, tmp, members, names, int(t), (m, n, gp, gp, gp, gp), flips_of[g["name"]], False) for t in ("0", "1", "2")}
            groups.append(dict(name=g["name"], scores=[m, n, gp], flips=flips_of[g["name"]], expected=exp))
        gaps = []
        for name in GAP_GROUPS:
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                names = [f"r{i}" for i in range(len(by_name[name]))]
                exp = {t: entry(libs, cli, tmp, by_name[name], names, int(t), scores, flips_of[name], False) for t in ("0", "1", "2")}
                gaps.append(dict(name=name, model=model, scores=list(scores), flips=flips_of[name], expected=exp))
        hand = []
        for name, mem, flips in hand_groups():
            members = [(s.encode(), None if q is None else q.encode()) for s, q in mem]
            names = [f"read{i}" for i in range(len(members))]
            exp = {t: entry(libs, cli, tmp, members, names, int(t), (5, -4, -8, -8, -8, -8), flips, True, True) for t in ("0", "1", "2")}
            hand.append(dict(name=name, scores=[5, -4, -8], seqs=[[s, q] for s, q in mem], flips=flips, expected=exp))
    every = [v for k in kat.values() for v in (k["plain"], k["strand"])] + \
            [v for g in groups + gaps + hand for t in ("0", "1", "2") for v in (g["expected"][t]["plain"], g["expected"][t]["strand"])]
    un = CHECK
    assert len(un) == len(every)
    assert any(r for e in un for _, r, _ in e["paths"]), "no reversed path"
    assert any(max(b - a for a, b in zip(e["out_off"], e["out_off"][1:])) >= 3 for e in un if e["edge_head"]), "no out-degree >= 3"

    def largest_block(e):
        n = {}
        for a, b in e["aligned"]:
            n[a] = n.get(a, 0) + 1
        return 1 + max(n.values(), default=0)
    assert any(largest_block(e) >= 3 for e in un), "no aligned block of 3 nodes"
    assert any(any(w % 2 for w in e["edge_weight"]) or any(w > 2 * len(e["paths"]) for w in e["edge_weight"]) for e in un), "no weights from qualities"
    hb = {g["name"]: g["expected"]["1"]["plain"] for g in hand}
    for k in (63, 64, 65):
        assert hb[f"nodes_{k}"]["counts"][0] == k, (k, hb[f"nodes_{k}"]["counts"])
    assert hb["members_70_of_20_bases"]["counts"][3] == 70
    od = G.unpack(hb["out_degree_4_and_aligned_column_of_4"]["tables"])
    assert max(b - a for a, b in zip(od["out_off"], od["out_off"][1:])) == 4 and largest_block(od) == 4
    assert sum(1 for e in every if "text" in e) >= 12 + 10
    rv0 = {g["name"]: g["expected"]["1"]["strand"] for g in hand}["reversed_member_0"]["tables"]
    assert not rv0["paths"][0][1] and any(r for _, r, _ in rv0["paths"])       # member 0 meets the empty graph: kept as given
    fx = dict(params=dict(generator="tests/golden/make_poa_graph.py",
                          reference="spoa's graph after the loop of src/main.cpp:277-316 and GenerateConsensus(), through the generator's "
                                    "own harness on oracle/_ref/libvcref_sisd.so (libvcref_sse41.so compared: simd_agrees); text: the "
                                    "stdout of spoa's own command line, -r 3 / -r 4 / -r 4 -s, and the file of -d",
                          sequences_from="tests/golden/sample.fastq.gz (kat), tests/golden/poa_groups.json.gz (groups, gaps); `strand`: "
                                         "the members of `flips` reverse-complemented, their quality reversed, before the call",
                          lists="first differences, tests/poa_graph_ref.unpack", digest="tests/poa_graph_ref.digest of the tables",
                          full_text_below=FULL_TEXT, full_tables_up_to_path_entries=FULL_TABLES),
              kat=kat, groups=groups, gaps=gaps, hand=hand)
    out = os.path.join(HERE, "poa_graph.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(every), "graphs,", sum(1 for e in every if "text" in e), "with text,",
          sum(1 for e in every if not e["simd_agrees"]), "where the SIMD build differs")


if __name__ == "__main__":
    main()
