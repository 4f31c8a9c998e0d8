"""TEST INFRASTRUCTURE: a CPU restatement of what spoa's graph keeps for, and returns from, the multiple sequence alignment and
the coverage summary, on top of tests/poa_gaps_ref.py (its Graph and Engine are imported, not edited) -- the bar for
vc_poa_run_msa beside the fixture tests/golden/poa_msa.json.gz, which comes from spoa itself.

  sequences_ and the edge labels                 <- vendor/spoa/src/graph.cpp:94-107 (AddEdge), 182-299 (AddAlignment)
  Node::Successor, Node::Coverage                <- graph.cpp:25-56
  InitializeMultipleSequenceAlignment            <- graph.cpp:393-413
  GenerateMultipleSequenceAlignment              <- graph.cpp:415-448
  GenerateConsensus(&summary, false)             <- graph.cpp:461-485

Everything is the reference's own loop: the Successor walk scans the out-edges and each edge's label list, Coverage builds the
set of labels.  Nothing here is trusted on its own: tests/test_poa_msa.py requires it to reproduce every fixture entry.
"""
import poa_gaps_ref as pg

CONSENSUS = 0xFFFFFFFF                                   # VC_POA_ROW_CONSENSUS


class MsaGraph(pg.Graph):
    def __init__(self):
        super().__init__()
        self.labels = []                                 # per edge, in the order added
        self.sequences = []                              # begin node of every sequence that was added
        self.members = []                                # its index among the calls of add_alignment (empty ones count)
        self._calls = 0

    def add_edge(self, t, h, w):
        for e in self.out[t]:
            if self.head[e] == h:
                self.weight[e] += w
                self.labels[e].append(len(self.sequences))
                return
        self.tail.append(t); self.head.append(h); self.weight.append(w)
        self.labels.append([len(self.sequences)])
        e = len(self.tail) - 1
        self.out[t].append(e); self.inn[h].append(e)

    def add_alignment(self, aln, seq, qual=None):
        """Graph::AddAlignment with sequences_: the base class's steps, keeping `begin`"""
        member, self._calls = self._calls, self._calls + 1
        n = len(seq)
        if n == 0:
            return                                       # before sequences_ grows (graph.cpp:187-190): no label, no row
        w = [1] * n if qual is None else [pg._LUT[b] for b in qual]
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
                    self.add_edge(prev, curr, (w[q - 1] + w[q]) & 0xFFFFFFFF)
                prev = curr
            if last is not None:
                self.add_edge(prev, last, (w[vback] + w[vback + 1]) & 0xFFFFFFFF)
        self.sequences.append(begin)
        self.members.append(member)
        self.toposort()

    # ------------------------------------------------------------------ Node::Successor / Node::Coverage
    def successor(self, v, label):
        for e in self.out[v]:
            if label in self.labels[e]:
                return self.head[e]
        return None

    def coverage_of(self, v):
        s = set()
        for e in self.inn[v]:
            s.update(self.labels[e])
        for e in self.out[v]:
            s.update(self.labels[e])
        return len(s)

    # ------------------------------------------------------------------ the outputs
    def columns(self):
        """InitializeMultipleSequenceAlignment -> (node -> column, row_size)"""
        dst = [0] * len(self.code)
        i = j = 0
        while i < len(self.rank):
            it = self.rank[i]
            dst[it] = j
            for a in self.aligned[it]:
                dst[a] = j
                i += 1
            i += 1
            j += 1
        return dst, j

    def consensus_path(self):
        """TraverseHeaviestBundle -> node ids (the base class's consensus(), keeping the nodes)"""
        if not self.rank:
            return []
        N = len(self.code)
        scores, pred = [-1] * N, [None] * N
        mx = None
        for it in self.rank:
            for e in self.inn[it]:
                if self._better(scores, pred, it, e):
                    scores[it], pred[it] = self.weight[e], self.tail[e]
            if pred[it] is not None:
                scores[it] += scores[pred[it]]
            if mx is None or scores[mx] < scores[it]:
                mx = it
        if self.out[mx]:
            node_rank = {v: r for r, v in enumerate(self.rank)}
            while self.out[mx]:
                mx = self._branch_completion(scores, pred, node_rank, node_rank[mx])
        path = [mx]
        while pred[mx] is not None:
            mx = pred[mx]
            path.append(mx)
        path.reverse()
        return path

    def msa(self, include_consensus):
        """GenerateMultipleSequenceAlignment -> (rows, members)"""
        col, row_size = self.columns()
        rows = []
        for i, it in enumerate(self.sequences):
            row = bytearray(b"-" * row_size)
            while it is not None:
                row[col[it]] = self.decoder[self.code[it]]
                it = self.successor(it, i)
            rows.append(bytes(row))
        members = list(self.members)
        if include_consensus:
            row = bytearray(b"-" * row_size)
            for v in self.consensus_path():
                row[col[v]] = self.decoder[self.code[v]]
            rows.append(bytes(row))
            members.append(CONSENSUS)
        return rows, members

    def summary(self):
        """GenerateConsensus(&summary, false) -> (consensus, coverage)"""
        path = self.consensus_path()
        cov = [self.coverage_of(v) + sum(self.coverage_of(a) for a in self.aligned[v]) for v in path]
        return bytes(self.decoder[self.code[v]] for v in path), cov


def msa(members, atype, m, n, g, e=None, q=None, c=None, include_consensus=True):
    """spoa's flow over one group: members = [(sequence bytes, quality bytes or None)]
    -> dict(rows, members, consensus, coverage)"""
    eng = pg.Engine(atype, m, n, g, e, q, c)
    gr = MsaGraph()
    for seq, qual in members:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
    rows, mem = gr.msa(include_consensus)
    cons, cov = gr.summary()
    assert cons == gr.consensus()
    return dict(rows=rows, members=mem, consensus=cons, coverage=cov)


def check_invariants(rows, members, group, include_consensus):
    """spoa's own checks after every known-answer run (test/spoa_test.cpp:54-76), on any MSA of `group`
    ([(sequence, quality or None)] or sequences): a row per non-empty member (+ 1), equal lengths, no column of gaps only, and
    every row without its gaps is its member"""
    seqs = [s[0] if isinstance(s, (tuple, list)) else s for s in group]
    nonempty = [i for i, s in enumerate(seqs) if len(s)]
    assert len(rows) == len(nonempty) + (1 if include_consensus else 0), (len(rows), len(nonempty))
    assert list(members) == nonempty + ([CONSENSUS] if include_consensus else []), members
    assert len({len(r) for r in rows}) <= 1
    for r, mb in zip(rows, members):
        if mb != CONSENSUS:
            assert bytes(r).replace(b"-", b"") == bytes(seqs[mb]), mb
    seq_rows = [r for r, mb in zip(rows, members) if mb != CONSENSUS]
    if seq_rows:
        for k in range(len(seq_rows[0])):
            assert any(r[k] != 0x2D for r in seq_rows), f"column {k} holds gaps only"
