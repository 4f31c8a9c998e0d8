"""Generates tests/golden/poa_gaps_groups.json.gz: the expected affine and convex consensus of the seeded groups of
poa_groups.json.gz (sizes 1 to 64, lengths 1 to 1 200 across k_lg_fwd's 512-column chunks, qualities, reverse complements, an
N / IUPAC read, repeats, empty sequences, an empty group, a local group that finds nothing), for all three algorithms and the
score sets below, from the CPU restatement tests/poa_gaps_ref.py.  The restatement is trusted because tests/test_poa_gaps.py
requires it to reproduce spoa's 18 known answers and every linear entry of poa_groups.json.gz; that test also recomputes entries
of this file.  The groups' sequences stay in poa_groups.json.gz; entries name them.

  python tests/golden/make_poa_gaps.py
"""
import gzip
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import poa_gaps_ref as R  # noqa: E402

# (match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2); the subtype follows spoa's rule
SCORES = {
    "affine_5_-4_-8_-6": (5, -4, -8, -6, -8, -6),             # spoa's affine known-answer tests
    "affine_2_-3_-5_0": (2, -3, -5, 0, -5, 0),                # free extension: long runs of equal scores
    "convex_5_-4_-8_-6_-10_-2": (5, -4, -8, -6, -10, -2),     # spoa's convex known-answer tests
    "convex_5_-4_-8_-6_-10_-4": (5, -4, -8, -6, -10, -4),     # spoa's command-line defaults
}


def load_groups():
    return json.load(gzip.open(os.path.join(HERE, "poa_groups.json.gz"), "rt"))["groups"]


def members(g):
    return [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]


def expected(g, t, scores):
    """-> {"status": 0 OK / 4 INVALID (the restatement throws), "consensus": str}"""
    try:
        return dict(status=0, consensus=R.consensus(members(g), t, *scores).decode())
    except ValueError:
        return dict(status=4, consensus="")


def _job(a):
    g, t, key = a
    return g["name"], t, key, expected(g, t, SCORES[key])


def main():
    groups = load_groups()
    jobs = [(g, t, key) for g in groups for t in (0, 1, 2) for key in SCORES]
    jobs.sort(key=lambda a: -sum(len(s) for s, _ in a[0]["seqs"]) * len(a[0]["seqs"]))
    out = {"scores": SCORES, "groups": {g["name"]: {} for g in groups}}
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        for name, t, key, e in ex.map(_job, jobs):
            out["groups"][name].setdefault(key, {})[str(t)] = e
    with gzip.open(os.path.join(HERE, "poa_gaps_groups.json.gz"), "wt", compresslevel=9) as f:
        json.dump(out, f, sort_keys=True)
    print(f"{len(jobs)} entries -> poa_gaps_groups.json.gz")


if __name__ == "__main__":
    main()
