"""TEST INFRASTRUCTURE: a CPU restatement of spoa's explicit-weight AddAlignment overloads and of the verbose summary of
GenerateConsensus, on top of tests/poa_msa_ref.py (imported, not edited) -- the bar for vc_poa_run_weighted beside the fixture
tests/golden/poa_weights.json.gz, which comes from spoa itself.

  AddAlignment(alignment, sequence, weight)      <- vendor/spoa/src/graph.cpp:132-147: one uint32 for every base
  AddAlignment(alignment, sequence, weights)     <- graph.cpp:174-300: weights[i - 1] + weights[i] in uint32, into an int64 edge
  GenerateConsensus(&summary, true)              <- graph.cpp:486-529: the literal walk with Successor(i) and the cursor c

A member's weight is None (the quality overload, or 1 for every base), an int (mode 1) or a list of ints (mode 2).  Nothing here
is trusted on its own: tests/test_poa_weights.py requires it to reproduce every fixture entry.
"""
import poa_gaps_ref as pg
import poa_msa_ref as pm
import poa_strand_ref as ps


def weight_vector(seq, qual, weight):
    """the std::vector<uint32_t> the reference's innermost AddAlignment receives"""
    n = len(seq)
    if weight is None:
        return [1] * n if qual is None else [pg._LUT[b] for b in qual]
    if isinstance(weight, int):
        return [weight] * n
    if len(weight) != n:
        raise ValueError("sequence and weights are of unequal size")      # graph.cpp:191-196
    return list(weight)


class WeightGraph(pm.MsaGraph):
    def add_weighted(self, aln, seq, qual=None, weight=None):
        """Graph::AddAlignment(alignment, sequence, sequence_len, weights), graph.cpp:182-299, behind the overload the member's
        weight selects: MsaGraph.add_alignment's steps with the weight vector given instead of looked up"""
        member, self._calls = self._calls, self._calls + 1
        n = len(seq)
        if n == 0:
            return                                       # before the size check and before sequences_ grows (graph.cpp:187-190)
        w = weight_vector(seq, qual, weight)
        for b in seq:
            if b not in self.coder:
                self.coder[b] = len(self.decoder)
                self.decoder.append(b)
        if not aln:
            begin = self._chain(seq, w, 0, n)
        else:
            qs = [q for _, q in aln if q != -1]
            if not qs:
                raise ValueError("invalid alignment")
            vfront, vback = qs[0], qs[-1]
            begin = self._chain(seq, w, 0, vfront)
            prev = len(self.code) - 1 if begin is not None else None
            last = self._chain(seq, w, vback + 1, n)
            for nd, q in aln:
                if q == -1:
                    continue
                c = self.coder[seq[q]]
                if nd == -1:
                    curr = self.add_node(c)
                elif self.code[nd] == c:
                    curr = nd
                else:
                    curr = next((a for a in self.aligned[nd] if self.code[a] == c), None)
                    if curr is None:
                        curr = self.add_node(c)
                        for a in list(self.aligned[nd]):
                            self.aligned[a].append(curr)
                            self.aligned[curr].append(a)
                        self.aligned[nd].append(curr)
                        self.aligned[curr].append(nd)
                if begin is None:
                    begin = curr
                if prev is not None:
                    self.add_edge(prev, curr, (w[q - 1] + w[q]) & 0xFFFFFFFF)      # uint32 sum, then into the int64 edge
                prev = curr
            if last is not None:
                self.add_edge(prev, last, (w[vback] + w[vback + 1]) & 0xFFFFFFFF)
        self.sequences.append(begin)
        self.members.append(member)
        self.toposort()

    def profile(self):
        """GenerateConsensus(&summary, true) -> (codes, counts): counts[k][c] as summary[k * consensus_.size() + c], gaps last"""
        path = self.consensus_path()
        nc, n = len(self.decoder), len(path)
        summary = [0] * ((nc + 1) * n)
        col, _ = self.columns()
        for i, it in enumerate(self.sequences):
            c, p, column, is_gap = 0, None, col[it], False
            while True:
                while c < n:
                    if col[path[c]] < column:
                        c += 1
                        continue
                    if col[path[c]] == column:
                        if is_gap:
                            for j in range(p + 1, c):
                                summary[nc * n + j] += 1
                        is_gap = True
                        p = c
                        summary[self.code[it] * n + c] += 1
                    break
                if c == n:
                    break
                it = self.successor(it, i)
                if it is None:
                    break
                column = col[it]
        return bytes(self.decoder), [summary[k * n:(k + 1) * n] for k in range(nc + 1)]

    def edges(self):
        """-> [(tail, head, weight)] by tail id, then by position in the tail's out-list (PoaGraph.edges' order)"""
        return [(t, self.head[e], self.weight[e]) for t in range(len(self.code)) for e in self.out[t]]


def build(members, weights, atype, m, n, g, e=None, q=None, c=None, strands=False):
    """spoa's flow over one group -> (WeightGraph, reversed flags): members = [(sequence bytes, quality bytes or None)], weights one
    entry per member (None, int or list).  strands: the -s loop (main.cpp:277-316); a kept reverse strand is added with its
    quality and its weight list reversed."""
    eng = ps.ScoreEngine(atype, m, n, g, e, q, c) if strands else pg.Engine(atype, m, n, g, e, q, c)
    gr = WeightGraph()
    rev = []
    for (seq, qual), wt in zip(members, weights):
        if not strands:
            gr.add_weighted(eng.align(seq, gr), seq, qual, wt)
            rev.append(0)
            continue
        rc = ps.reverse_complement(seq)
        (a, sa), (b, sb) = eng.align_score(seq, gr), eng.align_score(rc, gr)
        r = 0 if sa >= sb else 1
        ks, kq = ps.kept_view(seq, qual, r)
        gr.add_weighted(b if r else a, ks, kq, wt[::-1] if r and isinstance(wt, (list, tuple)) else wt)
        rev.append(r)
    return gr, rev


def run(members, weights, atype, m, n, g, e=None, q=None, c=None, strands=False):
    """-> dict(consensus, coverage, codes, counts, edges, rows, members, reversed)"""
    gr, rev = build(members, weights, atype, m, n, g, e, q, c, strands)
    cons, cov = gr.summary()
    codes, counts = gr.profile()
    rows, mem = gr.msa(False)
    return dict(consensus=cons, coverage=cov, codes=codes, counts=counts, edges=gr.edges(), rows=rows, members=mem, reversed=rev)


def counts_from_rows(rows, consensus_row, codes):
    """the profile re-derived from an MSA with its consensus row: for every consensus column the bytes of the member rows, and a
    gap where a member has bases on consensus columns on both sides -> counts as profile()'s"""
    cols = [k for k, ch in enumerate(consensus_row) if ch != 0x2D]
    idx = {b: k for k, b in enumerate(codes)}
    out = [[0] * len(cols) for _ in range(len(codes) + 1)]
    for r in rows:
        hits = [j for j, k in enumerate(cols) if r[k] != 0x2D]
        for j in hits:
            out[idx[r[cols[j]]]][j] += 1
        if hits:
            for j in range(hits[0], hits[-1] + 1):
                if r[cols[j]] == 0x2D:
                    out[len(codes)][j] += 1
    return out


def seeded_weights(members, seed, kind):
    """the weights of a fixture entry that records only (seed, kind): kind "seq" an int in 1..50 per member, "base" one int in 0..60
    per base, "mix" a mode 0 / 1 / 2 per member, "none" no weights"""
    import random
    rng = random.Random(seed)
    out = []
    for seq, _ in members:
        k = {"seq": 1, "base": 2, "mix": rng.randrange(3), "none": 0}[kind]
        out.append(None if k == 0 else rng.randint(1, 50) if k == 1 else [rng.randint(0, 60) for _ in seq])
    return out


def edge_digest(edges):
    import hashlib
    return hashlib.sha256(";".join("%d,%d,%d" % e for e in edges).encode()).hexdigest()
