"""Generates tests/golden/poa_assign.json.gz: every query of a list scored against the finished graph of EVERY group of a list
(vc_poa_run_assign, vechat_amd.poa.poa_assign) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the
reference tree lies (REF, as in oracle/Makefile).  The few lines of C++ below -- this generator's own -- are compiled in a
temporary directory against spoa's public headers and linked to oracle/_ref/libvcref_sisd.so (the SIMD build libvcref_sse41.so
compared: simd_agrees; the scalar build is the bar): the plain build loop of spoa's command line per group, then per query and
group `engine->Align(query, graph, &score)` as given and reverse-complemented (src/main.cpp:287-304 without the add).  Nothing
built is kept.

  python tests/golden/make_poa_assign.py

Every entry names its groups -- groups of tests/golden/poa_groups.json.gz by name, or `seqs` given in place --, its `queries`
and its six scores, and holds per algorithm ("0" kSW, "1" kNW, "2" kOV) `pairs[k][w] = [score, score_rev]` of query k against
group w.  Best, second and the kept strand follow from them by tests/poa_assign_ref.py, which the tests apply; the generator
applies it too, to assert that the fixture can fail: an entry whose best group is not group 0, one with a tie between two
groups, one with a reversed query kept, one where best and second differ by strand.
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

import poa_assign_ref as AR  # noqa: E402
from poa_strand_ref import reverse_complement  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SPOA = os.path.join(REF, "vendor", "spoa")
LINEAR, AFFINE, CONVEX = (5, -4, -8, -8, -8, -8), (5, -4, -8, -6, -8, -6), (5, -4, -8, -6, -10, -4)

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

// group w has the members first[w] .. first[w + 1] - 1.  out[2 * (k * ng + w)] = score, [.. + 1] = score of the reverse
// complement, of query k against group w.  Returns 0; -1: the reference threw
extern "C" int64_t assign_run(uint32_t ng, const uint32_t* first, const char* const* seqs, const uint32_t* lens, const char* const* quals,
                              uint32_t nq, const char* const* qseqs, const uint32_t* qlens, int type, int m, int n, int g, int e, int q,
                              int c, int64_t* out) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        for (uint32_t w = 0; w < ng; ++w) {
            spoa::Graph graph{};
            for (uint32_t i = first[w]; i < first[w + 1]; ++i) {
                std::string s(seqs[i], lens[i]);
                auto alignment = engine->Align(s, graph);
                if (quals[i]) graph.AddAlignment(alignment, s, std::string(quals[i], lens[i]));
                else graph.AddAlignment(alignment, s);
            }
            for (uint32_t k = 0; k < nq; ++k) {
                biosoup::Sequence it("q", 1, qseqs[k], qlens[k]);
                std::int32_t score = 0, score_rev = 0;
                engine->Align(it.data, graph, &score);
                it.ReverseAndComplement();
                engine->Align(it.data, graph, &score_rev);
                out[2 * ((uint64_t)k * ng + w)] = score;
                out[2 * ((uint64_t)k * ng + w) + 1] = score_rev;
            }
        }
        return 0;
    } catch (std::exception&) {
        return -1;
    }
}
"""


def build_reference(tmp):
    src = os.path.join(tmp, "assign_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    inc = [x for d in ("include", "src", "vendor/cereal/include", "vendor/bioparser/include", "vendor/bioparser/vendor/biosoup/include")
           for x in ("-I", os.path.join(SPOA, d))]
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"assign_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", *inc, src, "-o", out, so, "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].assign_run.restype = C.c_int64
    return libs


def run(lib, groups, queries, atype, scores):
    """-> pairs[k][w] = [score, score_rev], from the reference"""
    members = [m for g in groups for m in g]
    first = [0]
    for g in groups:
        first.append(first[-1] + len(g))
    k, nq, ng = len(members), len(queries), len(groups)
    SA, QA = C.c_char_p * max(k, 1), C.c_char_p * max(nq, 1)
    out = (C.c_int64 * max(2 * nq * ng, 1))()
    rc = lib.assign_run(C.c_uint32(ng), (C.c_uint32 * (ng + 1))(*first), SA(*[s for s, _ in members]),
                        (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members]), SA(*[q for _, q in members]), C.c_uint32(nq), QA(*queries),
                        (C.c_uint32 * max(nq, 1))(*[len(s) for s in queries]), C.c_int(atype), *[C.c_int(x) for x in scores], out)
    assert rc == 0, rc
    return [[[int(out[2 * (q * ng + w)]), int(out[2 * (q * ng + w) + 1])] for w in range(ng)] for q in range(nq)]


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


def entries(by_name):
    """[(entry name, [group name or inline members], [query], scores)]"""
    rng = random.Random(20250917)
    R = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))            # noqa: E731
    member = lambda name: rng.choice([s for s, _ in by_name[name] if s])  # noqa: E731
    fam = ["size3_len100_mixed", "size17_len200", "size8_len180_iupac", "empty_sequence_between", "low_qualities"]
    fam_q = [member(n) for n in fam] + [mutate(rng, member(fam[1])), reverse_complement(member(fam[2])), reverse_complement(mutate(rng, member(fam[4]))),
                                         R(120), b"", b"A"]
    small = ["size2_len12_fasta", "empty_group", "size3_len1_to_3", "homopolymers", "size2_len12_fasta", "empty_sequences_only"]
    small_q = [member("size2_len12_fasta"), member("homopolymers"), b"ACGT", b"", R(30)]
    base = R(90)
    fwd = [(base, None), (mutate(rng, base, 0.03), None)]
    back = [(reverse_complement(mutate(rng, base, 0.10)), None), (reverse_complement(mutate(rng, base, 0.10)), None)]
    other = [(R(90), None)]
    long_ = ["size17_len511", "size3_len513"]
    long_q = [member("size17_len511"), reverse_complement(member("size3_len513")), mutate(rng, member("size3_len513"))]
    out = []
    for model, sc in (("linear", LINEAR), ("affine", AFFINE), ("convex", CONVEX)):
        out.append((f"families_{model}", fam, fam_q, sc))
        out.append((f"strands_apart_{model}", [other, back, fwd], [base, mutate(rng, base), reverse_complement(base), R(40)], sc))
    out.append(("two_identical_groups_and_empty_ones", small, small_q, LINEAR))
    out.append(("chunk_edges_511_513", long_, long_q, AFFINE))
    return out


def main():
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    by_name = {g["name"]: [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]] for g in poa_fx["groups"]}
    fx_entries, seen = [], dict(not_group_0=False, tie=False, reversed_kept=False, strands_differ=False)
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_reference(tmp)
        for name, groups, queries, scores in entries(by_name):
            members = [by_name[g] if isinstance(g, str) else g for g in groups]
            exp = {}
            for t in (0, 1, 2):
                pairs = run(libs["sisd"], members, queries, t, scores)
                exp[str(t)] = dict(pairs=pairs, simd_agrees=run(libs["sse41"], members, queries, t, scores) == pairs)
                has_node = [any(s for s, _ in g) for g in members]
                for row in pairs:
                    both = [AR.kept(a, b) for a, b in row]
                    bg, bs, sg, ss = AR.rank_pairs([s for s, _ in both], has_node)
                    seen["not_group_0"] |= bg > 0
                    seen["tie"] |= bg >= 0 and sg >= 0 and bs == ss
                    seen["reversed_kept"] |= bg >= 0 and both[bg][1]
                    seen["strands_differ"] |= bg >= 0 and sg >= 0 and both[bg][1] != both[sg][1]
            fx_entries.append(dict(name=name, scores=list(scores),
                                   groups=[g if isinstance(g, str) else dict(seqs=[[s.decode(), q] for s, q in g]) for g in groups],
                                   queries=[s.decode("latin-1") for s in queries], expected=exp))
    assert all(seen.values()), seen                                        # the fixture can fail
    fx = dict(params=dict(generator="tests/golden/make_poa_assign.py",
                          reference="spoa's engine->Align(query, graph, &score) after the plain build loop of every group, as given and "
                                    "reverse-complemented, through the generator's own harness on oracle/_ref/libvcref_sisd.so "
                                    "(libvcref_sse41.so compared: simd_agrees)",
                          groups_from="tests/golden/poa_groups.json.gz by name, or `seqs` in place",
                          result="expected[type].pairs[query][group] = [score, score_rev]; best, second and strand by tests/poa_assign_ref.py"),
              entries=fx_entries)
    out = os.path.join(HERE, "poa_assign.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(fx_entries), "entries,",
          sum(len(e["queries"]) * len(e["groups"]) * 3 for e in fx_entries), "pairs,",
          sum(1 for e in fx_entries for x in e["expected"].values() if not x["simd_agrees"]), "runs where the SIMD build differs")


if __name__ == "__main__":
    main()
