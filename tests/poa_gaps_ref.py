"""TEST INFRASTRUCTURE: a CPU restatement of spoa's public flow with all three gap subtypes, the bar for vc_poa_run_gaps.

  AlignmentEngine::Create's subtype rule   <- vendor/spoa/src/alignment_engine.cpp:15-69
  SisdAlignmentEngine Initialize / Linear / Affine / Convex, WorstCaseAlignmentScore
                                            <- sisd_alignment_engine.cpp:117-925, alignment_engine.cpp:101-110
  Graph::AddAlignment, the topological sort, GenerateConsensus (heaviest bundle, branch completion)
                                            <- graph.cpp:132-300, 450-540 (restated as vechat_amd/csrc/vc_large.hip does)

The forward pass is vectorised over the columns of a row (numpy, int64): the vertical moves and the diagonal per predecessor
row, and the horizontal gaps as prefix maxima of tilted scores -- one scan for linear and affine rows, two passes for convex
rows (H from the scans over x, then E and Q over the final H); row_sequential() is spoa's own column loop for one row, and
tests/test_poa_gaps.py requires the two to agree.  The backtracks are spoa's loops, literally.  Nothing here is trusted on its
own: the CPU suite requires it to reproduce spoa's 18 known answers and every entry of tests/golden/poa_groups.json.gz.
"""
import numpy as np

KNEG = -2 ** 31 + 1024                                  # spoa's kNegativeInfinity
LINEAR, AFFINE, CONVEX = 0, 1, 2
SUBTYPES = {"linear": LINEAR, "affine": AFFINE, "convex": CONVEX}


def gap_model(g, e, q, c):
    """Create's rule -> (subtype, g, e, q, c) as the engine uses them"""
    if g >= e:
        return LINEAR, g, g, q, c
    if g <= q or e >= c:
        return AFFINE, g, e, g, e
    return CONVEX, g, e, q, c


def weight_lut():
    """graph.cpp:165-170 on a signed char quality, as uint32"""
    out = []
    for ch in range(256):
        q = ch - 256 if ch >= 128 else ch
        w = (1 - pow(10, (33 - q) / 10.)) * 1000
        out.append(int(w) & 0xFFFFFFFF)
    return out


_LUT = weight_lut()


# ------------------------------------------------------------------ the graph
class Graph:
    def __init__(self):
        self.code, self.inn, self.out, self.aligned = [], [], [], []
        self.tail, self.head, self.weight = [], [], []
        self.coder, self.decoder = {}, []
        self.rank = []

    def add_node(self, c):
        self.code.append(c)
        self.inn.append([]); self.out.append([]); self.aligned.append([])
        return len(self.code) - 1

    def add_edge(self, t, h, w):
        for e in self.out[t]:
            if self.head[e] == h:
                self.weight[e] += w
                return
        self.tail.append(t); self.head.append(h); self.weight.append(w)
        e = len(self.tail) - 1
        self.out[t].append(e); self.inn[h].append(e)

    def _chain(self, seq, w, begin, end):
        first = prev = None
        for i in range(begin, end):
            curr = self.add_node(self.coder[seq[i]])
            if first is None:
                first = curr
            if prev is not None:
                self.add_edge(prev, curr, (w[i - 1] + w[i]) & 0xFFFFFFFF)
            prev = curr
        return first

    def add_alignment(self, aln, seq, qual=None):
        n = len(seq)
        if n == 0:
            return
        w = [1] * n if qual is None else [_LUT[b] for b in qual]
        for b in seq:
            if b not in self.coder:
                self.coder[b] = len(self.decoder)
                self.decoder.append(b)
        if not aln:
            self._chain(seq, w, 0, n)
            self.toposort()
            return
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
        self.toposort()

    def toposort(self):
        N = len(self.code)
        marks, ignored, rank = [0] * N, [False] * N, []
        for s in range(N):
            if marks[s]:
                continue
            stack = [s]
            while stack:
                c = stack[-1]
                valid = True
                if marks[c] != 2:
                    for e in self.inn[c]:
                        t = self.tail[e]
                        if marks[t] != 2:
                            stack.append(t)
                            valid = False
                    if not ignored[c]:
                        for a in self.aligned[c]:
                            if marks[a] != 2:
                                stack.append(a)
                                ignored[a] = True
                                valid = False
                    if valid:
                        marks[c] = 2
                        if not ignored[c]:
                            rank.append(c)
                            rank.extend(self.aligned[c])
                    else:
                        marks[c] = 1
                if valid:
                    stack.pop()
        self.rank = rank

    def _better(self, scores, pred, it, e):
        tl = self.tail[e]
        return scores[it] < self.weight[e] or (scores[it] == self.weight[e] and pred[it] is not None and scores[pred[it]] <= scores[tl])

    def _branch_completion(self, scores, pred, node_rank, r):
        start = self.rank[r]
        for o in self.out[start]:
            for e in self.inn[self.head[o]]:
                if self.tail[e] != start:
                    scores[self.tail[e]] = -1
        mx = None
        for i in range(r + 1, len(self.rank)):
            it = self.rank[i]
            scores[it], pred[it] = -1, None
            for e in self.inn[it]:
                if scores[self.tail[e]] == -1:
                    continue
                if self._better(scores, pred, it, e):
                    scores[it], pred[it] = self.weight[e], self.tail[e]
            if pred[it] is not None:
                scores[it] += scores[pred[it]]
            if mx is None or scores[mx] < scores[it]:
                mx = it
        return mx

    def consensus(self):
        if not self.rank:
            return b""
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
        return bytes(self.decoder[self.code[v]] for v in reversed(path))


# ------------------------------------------------------------------ one row's horizontal gaps
def _excl(v0, x, d, g):
    """E[j] for j = 1 .. len: max(max_k<j (v[k] + g + (j - 1 - k) d), KNEG + j d), v[0] = v0, v[k] = x[k - 1]"""
    n = x.shape[0]
    j = np.arange(n + 1, dtype=np.int64)
    t = np.empty(n + 1, np.int64)
    t[0] = max(v0, KNEG - g + d)
    t[1:] = x - j[1:] * d
    return np.maximum.accumulate(t)[:-1] + (g - d) + j[1:] * d


def row_scan(sub, x, h0, g, e, q, c):
    """H, E, Q of columns 1 .. len from x = max(diagonal, F (, O) (, 0 for kSW)) and H[i][0] = h0 (E, Q: None where the subtype
    has none).  Linear: H = x then prefix maximum with g.  Affine: E from one scan over x (equal to the scan over H since g <= e),
    H = max(x, E).  Convex: H from the scans over x with (g, e) and (q, c); E and Q scanned again over the final H."""
    x = np.asarray(x, np.int64)
    if sub == LINEAR:
        n = x.shape[0]
        j = np.arange(n + 1, dtype=np.int64)
        t = np.empty(n + 1, np.int64)
        t[0] = h0
        t[1:] = x - j[1:] * g
        return np.maximum.accumulate(t)[1:] + j[1:] * g, None, None
    E = _excl(h0, x, e, g)
    if sub == AFFINE:
        return np.maximum(x, E), E, None
    H = np.maximum(x, np.maximum(E, _excl(h0, x, c, q)))
    return H, _excl(h0, H, e, g), _excl(h0, H, c, q)


def row_sequential(sub, sw, d, f, o, h0, g, e, q, c):
    """spoa's own loop over the columns of one row (Linear / Affine / Convex after the predecessors): d the diagonal maximum,
    f / o the vertical ones (f: linear's H_pred + g) -> H, E, Q (lists, columns 1 .. len)"""
    n = len(d)
    H, E, Q = [h0] + list(d), [KNEG] + [0] * n, [KNEG] + [0] * n
    for j in range(1, n + 1):
        if sub == LINEAR:
            H[j] = max(H[j - 1] + g, max(d[j - 1], f[j - 1]))
        else:
            E[j] = max(H[j - 1] + g, E[j - 1] + e)
            h = max(H[j], max(f[j - 1], E[j]))
            if sub == CONVEX:
                Q[j] = max(H[j - 1] + q, Q[j - 1] + c)
                h = max(h, max(o[j - 1], Q[j]))
            H[j] = h
        if sw:
            H[j] = max(H[j], 0)
    return H[1:], (E[1:] if sub != LINEAR else None), (Q[1:] if sub == CONVEX else None)


# ------------------------------------------------------------------ the engine
def worst_case(m, g, e, q, c, i, j):
    def gs(n):
        return 0 if n == 0 else min(g + (n - 1) * e, q + (n - 1) * c)
    return min(-1 * (m * min(i, j) + gs(abs(i - j))), gs(i) + gs(j))


class Engine:
    def __init__(self, atype, m, n, g, e=None, q=None, c=None):
        e = g if e is None else e
        q = g if q is None else q
        c = e if c is None else c
        if atype not in (0, 1, 2):
            raise ValueError("invalid alignment type")
        if g > 0 or q > 0 or e > 0 or c > 0:
            raise ValueError("gap penalties must be non-positive")
        self.type, self.m, self.n = atype, m, n
        self.sub, self.g, self.e, self.q, self.c = gap_model(g, e, q, c)

    def align(self, seq, graph):
        """-> list of (node id or -1, position or -1)"""
        N, L = len(graph.rank), len(seq)
        if N == 0 or L == 0:
            return []
        if worst_case(self.m, self.g, self.e, self.q, self.c, L, N) < KNEG:
            raise ValueError("possible overflow")
        sub, sw, nw, ov = self.sub, self.type == 0, self.type == 1, self.type == 2
        g, e, q, c, w = self.g, self.e, self.q, self.c, L + 1
        node_rank = {v: r for r, v in enumerate(graph.rank)}
        preds = [[node_rank[graph.tail[x]] + 1 for x in graph.inn[v]] for v in graph.rank]
        s = np.frombuffer(bytes(seq), np.uint8)
        jj = np.arange(1, w, dtype=np.int64)
        H = np.zeros((N + 1, w), np.int64)
        F = E = O = Q = None
        # Initialize
        if sub != LINEAR:
            F, E = np.zeros_like(H), np.zeros_like(H)
            F[0, 1:] = KNEG
            E[0, 1:] = g + (jj - 1) * e
            E[1:, 0] = KNEG
        if sub == CONVEX:
            O, Q = np.zeros_like(H), np.zeros_like(H)
            O[0, 1:] = KNEG
            Q[0, 1:] = q + (jj - 1) * c
            Q[1:, 0] = KNEG
        if not sw:
            H[0, 1:] = jj * g if sub == LINEAR else (E[0, 1:] if sub == AFFINE else np.maximum(Q[0, 1:], E[0, 1:]))
        best, bi, bj = (0 if sw else KNEG), 0, 0
        for r, v in enumerate(graph.rank):
            i = r + 1
            ps = preds[r] or [0]
            if sub != LINEAR:                                   # column 0 of F (and O): chains over the predecessors
                F[i, 0] = (max(F[p, 0] for p in preds[r]) if preds[r] else g - e) + e
                if sub == CONVEX:
                    O[i, 0] = (max(O[p, 0] for p in preds[r]) if preds[r] else q - c) + c
            if nw:
                if sub == LINEAR:
                    H[i, 0] = (max(H[p, 0] for p in preds[r]) if preds[r] else 0) + g
                else:
                    H[i, 0] = F[i, 0] if sub == AFFINE else max(O[i, 0], F[i, 0])
            prof = np.where(s == graph.decoder[graph.code[v]], self.m, self.n).astype(np.int64)
            d = f = o = None
            for p in ps:
                dp = H[p, :-1] + prof
                fp = H[p, 1:] + g if sub == LINEAR else np.maximum(H[p, 1:] + g, F[p, 1:] + e)
                d = dp if d is None else np.maximum(d, dp)
                f = fp if f is None else np.maximum(f, fp)
                if sub == CONVEX:
                    op = np.maximum(H[p, 1:] + q, O[p, 1:] + c)
                    o = op if o is None else np.maximum(o, op)
            x = np.maximum(d, f)
            if sub == CONVEX:
                x = np.maximum(x, o)
                O[i, 1:] = o
            if sub != LINEAR:
                F[i, 1:] = f
            if sw:
                x = np.maximum(x, 0)
            h, eh, qh = row_scan(sub, x, int(H[i, 0]), g, e, q, c)
            H[i, 1:] = h
            if eh is not None:
                E[i, 1:] = eh
            if qh is not None:
                Q[i, 1:] = qh
            sink = not graph.out[v]
            if sw or (ov and sink):
                k = int(np.argmax(h))
                if h[k] > best:
                    best, bi, bj = int(h[k]), i, k + 1
            elif nw and sink and h[-1] > best:
                best, bi, bj = int(h[-1]), i, L
        if bi == 0 and bj == 0:
            return []
        return self._backtrack(graph, seq, preds, H, F, E, O, Q, bi, bj)

    def _backtrack(self, graph, seq, preds, H, F, E, O, Q, i, j):
        sub, sw, ov = self.sub, self.type == 0, self.type == 2
        g, e, q, c = self.g, self.e, self.q, self.c
        H, F, E, O, Q = (None if a is None else a.tolist() for a in (H, F, E, O, Q))
        aln = []
        while True:
            if sw:
                if H[i][j] == 0:
                    break
            elif ov:
                if i == 0 or j == 0:
                    break
            elif i == 0 and j == 0:
                break
            Hij = H[i][j]
            cand = (preds[i - 1] or [0]) if i else []
            found = up = left = False
            pi = pj = 0
            if i != 0 and j != 0:
                s = self.m if seq[j - 1] == graph.decoder[graph.code[graph.rank[i - 1]]] else self.n
                for p in cand:
                    if Hij == H[p][j - 1] + s:
                        pi, pj, found = p, j - 1, True
                        break
            if not found and i != 0:
                for p in cand:
                    if sub == LINEAR:
                        found = Hij == H[p][j] + g
                    elif sub == AFFINE:
                        up = Hij == F[p][j] + e
                        found = up or Hij == H[p][j] + g
                    else:
                        up = Hij == F[p][j] + e
                        if not up and Hij != H[p][j] + g:
                            up = Hij == O[p][j] + c
                        found = up or Hij == H[p][j] + g or Hij == H[p][j] + q
                    if found:
                        pi, pj = p, j
                        break
            if not found and j != 0:
                if sub == LINEAR:
                    found = Hij == H[i][j - 1] + g
                elif sub == AFFINE:
                    left = Hij == E[i][j - 1] + e
                    found = left or Hij == H[i][j - 1] + g
                else:
                    left = Hij == E[i][j - 1] + e
                    if not left and Hij != H[i][j - 1] + g:
                        left = Hij == Q[i][j - 1] + c
                    found = left or Hij == H[i][j - 1] + g or Hij == H[i][j - 1] + q
                if found:
                    pi, pj = i, j - 1
            if not found:
                raise RuntimeError("no predecessor")
            aln.append((-1 if i == pi else graph.rank[i - 1], -1 if j == pj else j - 1))
            i, j = pi, pj
            if left:
                while True:
                    aln.append((-1, j - 1))
                    j -= 1
                    if sub == AFFINE:
                        if E[i][j] + e != E[i][j + 1]:
                            break
                    elif E[i][j] + e != E[i][j + 1] and Q[i][j] + c != Q[i][j + 1]:
                        break
            elif up:
                while True:
                    prev = 0
                    if sub == AFFINE:
                        stop = False
                        for p in preds[i - 1]:
                            stop = F[i][j] == H[p][j] + g
                            if stop or F[i][j] == F[p][j] + e:
                                prev = p
                                break
                    else:
                        stop = True
                        for p in preds[i - 1]:
                            if F[i][j] == F[p][j] + e or O[i][j] == O[p][j] + c:
                                prev, stop = p, False
                                break
                        if stop:
                            for p in preds[i - 1]:
                                if F[i][j] == H[p][j] + g or O[i][j] == H[p][j] + q:
                                    prev = p
                                    break
                    aln.append((graph.rank[i - 1], -1))
                    i = prev
                    if stop or i == 0:
                        break
        aln.reverse()
        return aln


def consensus(members, atype, m, n, g, e=None, q=None, c=None):
    """spoa's flow over one group: members = [(sequence bytes, quality bytes or None)] -> consensus bytes"""
    eng = Engine(atype, m, n, g, e, q, c)
    gr = Graph()
    for seq, qual in members:
        gr.add_alignment(eng.align(seq, gr), seq, qual)
    return gr.consensus()
