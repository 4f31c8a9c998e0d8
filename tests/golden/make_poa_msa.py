"""Generates tests/golden/poa_msa.json.gz: the multiple sequence alignment and the coverage summary of POA groups
(vc_poa_run_msa, vechat_amd.poa.poa_msa) from the REAL reference.  Runs where oracle/_ref was built (after build()) and the
reference tree lies (REF, as in oracle/Makefile): the few lines of C++ below -- this generator's own
-- are compiled against spoa's public headers and linked to oracle/_ref/libvcref_sisd.so (spoa's scalar engines) and to
libvcref_sse41.so (the SIMD build) in a temporary directory, and call, per entry,

    AlignmentEngine::Create(type, m, n, g, e, q, c); Align + AddAlignment per member;
    GenerateMultipleSequenceAlignment(true); GenerateConsensus(&summary, false)

  python tests/golden/make_poa_msa.py

Entries:
  kat     spoa's known-answer flow on the 55 reads of sample.fastq.gz, every entry of spoa_kat_gaps.json (the three algorithms
          at 5/-4/-8 linear, -8/-6 affine and -8/-6/-10/-2 convex, with and without qualities); the consensus must equal the
          committed one, so it is the same run;
  groups  the seeded groups of poa_groups.json.gz, re-read from that file, all three algorithms at the group's scores; the
          consensus must equal the committed one;
  gaps    five of those groups (one with an empty member) at one affine and one convex score set of poa_gaps_groups.json.gz,
          all three algorithms; the consensus must equal the one committed there.
Every entry holds rows (the last one the consensus row), members (the group member of every sequence row) and coverage, in
full, from the SCALAR build: the device restates spoa's scalar engines (sisd_alignment_engine.cpp).  With linear and affine gaps
the SIMD build must give the same MSA wherever it gives the same consensus.  With convex gaps it does not: on the 55 reads the
two builds return the same consensus from different, equally scoring alignments (e.g. 909 against 895 columns, kSW at
-8/-6/-10/-2), and so they do on one linear entry, the group "local_finds_nothing" under kOV (unrelated members: every end
cell ties; 26 against 28 columns).  For these `simd_agrees` only records what was seen; everywhere else it is asserted.
"""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fixtures  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
TYPES = {"SW": 0, "NW": 1, "OV": 2}
GAP_SETS = {"affine": "affine_5_-4_-8_-6", "convex": "convex_5_-4_-8_-6_-10_-4"}       # score sets of poa_gaps_groups.json.gz
GAP_GROUPS = ("size3_len100_mixed", "size17_len200", "size12_len400_revcomp", "size8_len180_iupac", "empty_sequence_between")

HARNESS = r"""
#include <cstdint>
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include "spoa/spoa.hpp"

// rows: n_rows x row_size bytes back to back; -1: the reference threw; -2: a buffer is too small
extern "C" int msa_run(uint32_t k, const char* const* seqs, const uint32_t* lens, const char* const* quals, int type,
                       int m, int n, int g, int e, int q, int c, char* rows, uint64_t rows_cap, uint32_t* n_rows,
                       uint32_t* row_size, char* cons, uint32_t cons_cap, uint32_t* cons_len, uint32_t* coverage) {
    try {
        auto engine = spoa::AlignmentEngine::Create(static_cast<spoa::AlignmentType>(type), m, n, g, e, q, c);
        spoa::Graph graph{};
        for (uint32_t i = 0; i < k; ++i) {
            auto alignment = engine->Align(seqs[i], lens[i], graph);
            if (quals[i]) graph.AddAlignment(alignment, seqs[i], lens[i], quals[i], lens[i]);
            else graph.AddAlignment(alignment, seqs[i], lens[i]);
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
    src = os.path.join(tmp, "msa_harness.cpp")
    open(src, "w").write(HARNESS)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    libs = {}
    for kind in ("sisd", "sse41"):
        so = os.path.join(ref_dir, f"libvcref_{kind}.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run build() where the reference tree is present")
        out = os.path.join(tmp, f"msa_{kind}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(REF, "vendor/spoa/include"),
                               "-I", os.path.join(REF, "vendor/spoa/vendor/cereal/include"), src, "-o", out, so,
                               "-Wl,-rpath," + ref_dir])
        libs[kind] = C.CDLL(out)
        libs[kind].msa_run.restype = C.c_int
    return libs


def run(lib, members, atype, scores):
    """members [(bytes, bytes | None)] -> (rc, rows, consensus, coverage)"""
    k = len(members)
    SA = C.c_char_p * max(k, 1)
    sa = SA(*[s for s, _ in members])
    qa = SA(*[q for _, q in members])
    la = (C.c_uint32 * max(k, 1))(*[len(s) for s, _ in members])
    total = sum(len(s) for s, _ in members)
    cap = (k + 1) * (total + 1)
    rows = C.create_string_buffer(max(cap, 1))
    cons = C.create_string_buffer(total + 1)
    cov = (C.c_uint32 * (total + 1))()
    n_rows, row_size, cons_len = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib.msa_run(C.c_uint32(k), sa, la, qa, C.c_int(atype), *[C.c_int(x) for x in scores], rows, C.c_uint64(cap),
                     C.byref(n_rows), C.byref(row_size), cons, C.c_uint32(total + 1), C.byref(cons_len), cov)
    if rc != 0:
        return rc, [], b"", []
    rs = row_size.value
    return 0, [rows.raw[i * rs:(i + 1) * rs] for i in range(n_rows.value)], cons.raw[:cons_len.value], list(cov[:cons_len.value])


def entry(libs, members, atype, scores, want_consensus, tie_case=False):
    """one fixture entry from the scalar build, compared with the SIMD one and with the committed consensus"""
    rc, rows, cons, cov = run(libs["sisd"], members, atype, scores)
    assert rc == 0, rc
    rc2, rows2, cons2, cov2 = run(libs["sse41"], members, atype, scores)
    assert rc2 == 0, rc2
    simd_agrees = (rows2, cov2) == (rows, cov)
    g, e, q, c = scores[2:]
    convex = g < e and not (g <= q or e >= c)              # Create's subtype rule (alignment_engine.cpp:59-69)
    if cons2 == cons and not convex and not (tie_case and atype == 2):
        assert simd_agrees, "the SIMD and scalar builds agree on the consensus but not on the MSA"
    assert cons == want_consensus, "not the run of the committed consensus"
    nonempty = [i for i, (s, _) in enumerate(members) if len(s)]
    assert len(rows) == len(nonempty) + 1
    for r, i in zip(rows, nonempty):
        assert r.replace(b"-", b"") == members[i][0]
    assert rows[-1].replace(b"-", b"") == cons
    return dict(rows=[r.decode() for r in rows], members=nonempty, consensus=cons.decode(), coverage=cov, simd_agrees=simd_agrees)


def main():
    seqs, quals = fixtures.load_sample_reads()
    poa_fx = json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))
    gaps_fx = json.load(gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "rt"))
    with tempfile.TemporaryDirectory() as tmp:
        libs = build_harness(tmp)
        kat = {}
        for name, k in json.load(open(os.path.join(HERE, "spoa_kat_gaps.json"))).items():
            members = list(zip(seqs, quals if k["quality"] else [None] * len(seqs)))
            scores = (k["m"], k["n"], k["g"], k["e"], k["q"], k["c"])
            kat[name] = dict(type=k["type"], scores=list(scores), quality=k["quality"],
                             **entry(libs, members, TYPES[k["type"]], scores, k["consensus"].encode()))
        groups, by_name = [], {}
        for g in poa_fx["groups"]:
            members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
            by_name[g["name"]] = members
            m, n, gp = g["scores"]
            exp = {}
            for t in ("0", "1", "2"):
                assert g["expected"][t]["status"] == 0, g["name"]
                exp[t] = entry(libs, members, int(t), (m, n, gp, gp, gp, gp), g["expected"][t]["consensus"].encode(),
                               tie_case=g["name"] == "local_finds_nothing")
            groups.append(dict(name=g["name"], scores=[m, n, gp], expected=exp))
        gaps = []
        for name in GAP_GROUPS:
            for model, key in GAP_SETS.items():
                scores = tuple(gaps_fx["scores"][key])
                exp = {}
                for t in ("0", "1", "2"):
                    want = gaps_fx["groups"][name][key][t]
                    assert want["status"] == 0, (name, key, t)
                    exp[t] = entry(libs, by_name[name], int(t), scores, want["consensus"].encode())
                gaps.append(dict(name=name, model=model, scores=list(scores), expected=exp))
    fx = dict(params=dict(generator="tests/golden/make_poa_msa.py",
                          reference="spoa::Graph of oracle/_ref/libvcref_sisd.so through the generator's own harness; "
                                    "libvcref_sse41.so agreeing",
                          groups_from="tests/golden/poa_groups.json.gz (sequences are not repeated here)"),
              kat=kat, groups=groups, gaps=gaps)
    out = os.path.join(HERE, "poa_msa.json.gz")
    with gzip.open(out, "wt", compresslevel=9) as f:
        json.dump(fx, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(kat), "known answers,", len(groups), "groups x 3,", len(gaps), "gap entries x 3")


if __name__ == "__main__":
    main()
