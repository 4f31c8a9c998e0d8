"""TEST INFRASTRUCTURE: a CPU restatement of spoa's strand-ambiguous flow (`-s`), the bar for vc_poa_run_strand beside the
fixture tests/golden/poa_strand.json.gz, which comes from spoa itself.  On top of tests/poa_gaps_ref.py (the engine) and
tests/poa_msa_ref.py (the graph with its rows and coverage); both are imported, not edited.

  the loop over the sequences, the choice           <- vendor/spoa/src/main.cpp:277-316
  Sequence::ReverseAndComplement                    <- biosoup/sequence.hpp:55-77
  where the engine writes *score                    <- sisd_alignment_engine.cpp:362-367 (and the affine / convex twins)

The complement of a byte is looked up on its upper-cased form and is upper case: A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H.
Every other byte -- S, W, N among them -- has no entry and stays as it is, in its own case.  So complementing twice (what
happens to a kept forward strand) maps u / U to T and lower-case a c g t r y k m b d h v to upper case, and nothing else.
The score of an alignment is the end cell's value; it is written only where the engine reaches its backtrack, so it stays 0
against an empty graph, for an empty sequence, and for a local alignment without a positive cell.
Nothing here is trusted on its own: tests/test_poa_strand.py requires it to reproduce every fixture entry.
"""
import poa_gaps_ref as pg
import poa_msa_ref as pm

_PAIRS = ("AT", "CG", "RY", "KM", "BV", "DH")
_UPPER = {ord(a): ord(b) for a, b in _PAIRS}
_UPPER.update({ord(b): ord(a) for a, b in _PAIRS})
_UPPER[ord("U")] = ord("A")


def complement_byte(c):
    up = c - 32 if 0x61 <= c <= 0x7A else c
    return _UPPER.get(up, c)


COMPLEMENT = bytes(complement_byte(c) for c in range(256))
ROUND_TRIP = bytes(COMPLEMENT[COMPLEMENT[c]] for c in range(256))


def reverse_complement(seq):
    return bytes(seq).translate(COMPLEMENT)[::-1]


def round_trip(seq):
    """what two calls of ReverseAndComplement leave of a sequence"""
    return bytes(seq).translate(ROUND_TRIP)


def kept_view(seq, qual, reversed_):
    """the bytes and quality string that are added for a member, given the choice"""
    if reversed_:
        return reverse_complement(seq), None if qual is None else bytes(qual)[::-1]
    return round_trip(seq), qual


class ScoreEngine(pg.Engine):
    """pg.Engine that also returns spoa's *score: the end cell's value where the backtrack is reached, else 0"""

    def align_score(self, seq, graph):
        self._score = 0
        aln = self.align(seq, graph)
        return aln, self._score

    def _backtrack(self, graph, seq, preds, H, F, E, O, Q, i, j):
        self._score = int(H[i][j])
        return super()._backtrack(graph, seq, preds, H, F, E, O, Q, i, j)


def strands(members, atype, m, n, g, e=None, q=None, c=None, include_consensus=True):
    """spoa's flow with -s over one group: members = [(sequence bytes, quality bytes or None)]
    -> dict(reversed, score, score_rev (one entry per member), kept (the members as added), rows, members, consensus, coverage)"""
    eng = ScoreEngine(atype, m, n, g, e, q, c)
    gr = pm.MsaGraph()
    rev, sc, scr, kept = [], [], [], []
    for seq, qual in members:
        seq = bytes(seq)
        aln, s0 = eng.align_score(seq, gr)
        aln_r, s1 = eng.align_score(reverse_complement(seq), gr)
        r = not s0 >= s1                                 # ties keep the forward strand
        ks, kq = kept_view(seq, qual, r)
        gr.add_alignment(aln_r if r else aln, ks, kq)
        rev.append(r); sc.append(s0); scr.append(s1); kept.append((ks, kq))
    rows, mem = gr.msa(include_consensus)
    cons, cov = gr.summary()
    assert cons == gr.consensus()
    return dict(reversed=rev, score=sc, score_rev=scr, kept=kept, rows=rows, members=mem, consensus=cons, coverage=cov)
