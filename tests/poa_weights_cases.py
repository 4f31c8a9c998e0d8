"""TEST INFRASTRUCTURE: the entries of tests/golden/poa_weights.json.gz as (id, members, weights, type, scores, strands, expected),
shared by tests/test_poa_weights.py and tests/test_poa_weights_gpu.py."""
import gzip
import json
import os

import fixtures
import poa_strand_ref as ps
import poa_weights_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return json.load(gzip.open(os.path.join(GOLDEN, "poa_weights.json.gz"), "rt"))


def cases(fx=None):
    fx = fx or load()
    groups = {g["name"]: [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
              for g in json.load(gzip.open(os.path.join(GOLDEN, "poa_groups.json.gz"), "rt"))["groups"]}
    seqs, _ = fixtures.load_sample_reads()
    plain = [(s, None) for s in seqs]
    lin = lambda sc: tuple(sc) + (sc[2],) * 3 if len(sc) == 3 else tuple(sc)      # noqa: E731
    out = []
    for k in fx["kat"]:
        out.append((f"kat-{k['kind']}-{k['type']}", plain, W.seeded_weights(plain, k["seed"], k["kind"]), k["type"], lin(k["scores"]), False, k["expected"]))
    for sect in ("groups", "gaps", "strand", "hand"):
        for g in fx[sect]:
            if sect == "hand":
                members = [(s.encode(), None if q is None else q.encode()) for s, q in g["seqs"]]
                weights = g["weights"]
            else:
                members = groups[g["name"]]
                if sect == "strand":
                    fl = set(g["flips"])
                    members = [(ps.reverse_complement(s), None if q is None else q[::-1]) if i in fl else (s, q) for i, (s, q) in enumerate(members)]
                weights = W.seeded_weights(members, g["seed"], g["kind"])
            for t, e in g["expected"].items():
                out.append((f"{sect}-{g['name']}-{g.get('model', 'linear')}-{t}", members, weights, int(t), lin(g["scores"]), sect == "strand", e))
    return out


def check(got, e, what):
    """got: dict(consensus, codes, counts, edges[, reversed]) with bytes / lists; e: the fixture entry"""
    assert got["consensus"] == e["consensus"].encode("latin-1"), what
    assert got["codes"] == e["codes"].encode("latin-1"), what
    assert [list(map(int, r)) for r in got["counts"]] == e["counts"], what
    edges = [tuple(int(v) for v in x) for x in got["edges"]]
    assert len(edges) == e["n_edges"] and W.edge_digest(edges) == e["edge_digest"], what
    if "edges" in e:
        assert [list(x) for x in edges] == e["edges"], what
    if "reversed" in e:
        assert [int(x) for x in got["reversed"]] == e["reversed"], what
