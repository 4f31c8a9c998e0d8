"""TEST INFRASTRUCTURE: the case table of the stored band, the row records and the backtrack (tests/test_trace_cases.py on the CPU,
tests/test_trace_cases_gpu.py on the device), beside tests/fwd_cases.py, whose window / Scores / Case machinery it uses.

CHAIN-PLUS-SKIP GRAPHS.  A graph that contains a Hamiltonian path has exactly one topological order.  A window whose layers differ from
the backbone only by deletions gives the backbone chain plus skip edges, so in every valid order -- the reference's rank and the
library's incremental VcGraph::ord alike -- row r is backbone position r (rows count from 1; row 0 is the virtual row), the first
in-edge of every row is the chain edge, and every in-degree, list position and row distance is what chain_graph() says.  The PROBE is
the last layer (Batch.from_windows(..., presorted=True)): it may carry anything, nothing is aligned after it in the racon-linear overload.

WHICH LAUNCHES ARE BANDED (vc_api.hip: vc_submit's `bt->band = bt->packed && bt->kept`, Plan::fwd_args / trace_args, Plan::redo,
Plan::finish): a batch is banded when both score sets pass vc_row_packed at the batch's widest class and the row capacity is below
32 768 (kept-row ring on).  Then the build phase's forward launches (fa.mode == 0) and the re-alignment launches (fa.mode == 1; these
are VcFwdArgs::mode, the phase of a launch, not the overload `mode` of the parameters that the tests pass) store the band of
every GLOBAL alignment (VcFwdArgs::band; k_tracew: `band = a.band && !redo && type == 1`); local alignments, the final local alignment
of the backbone (fa.band = 0), redo passes (whole rows) and raw int16 rows (classes of 32 and more columns per lane under the shipped
scores) are never banded.  VcTraceArgs::band_chain is set for the re-alignment rounds, but VC_BAND_CHAIN_COLS is 0 in the product: the
width is vc_band_lanes(cpl) in both phases.  banded() below restates this.

THE BAND OF A ROW (vc_kernels.h).  An alignment of `length` columns against `nrows` rows in class cpl has the slope
ql = min(((length << 16) // nrows) // cpl, 0xFFFFFF) (16.16 lanes per row); rows 16 b + 1 .. 16 b + 16 store the bl = band_lanes(cpl)
lanes from band_start(16 b + 9): t = (row * ql) >> 16 (24-bit multiply), min(max(t, bl/2 - 1) - (bl/2 - 1), 64 - bl).  Lane l holds
columns l * cpl + 1 .. (l + 1) * cpl; row 0 and column 0 are not stored in the band and always available.

CLASSIFICATION of one global alignment (path = the cells the reference's backtrack visits):
  outside: a path cell is not in the band.  The walk reads every path cell (as a speculated cell, which then confirms nothing and hands
           the position to the general step, or as a candidate of a general step): it raises oob and the alignment is redone.
  clear:   for every path cell (r, c) and every predecessor row pr of r, the cells (pr, c - 1), (pr, c) and (r, c - 1) are in the band.
           The general step at (r, c) reads exactly T[pr][c - 1] (diagonal), T[pr][c] (vertical) for listed predecessors and
           T[r][c - 1] (horizontal); the speculation reads T[first predecessor][c - 1] only: a subset.  Nothing else is read, so such an
           alignment cannot be redone.
  unclear: anything else.  Cases marked exact hold none; there band_redo == number of outside alignments in the linear overload.

KEPT RING (vc_frec_kept; K = kKept = VC_KEPT = 6 slots in vc_api.hip for classes below 32 columns per lane, kKeptWide = 3 from there):
rows that some row reads at distance 2 .. 64 are `kept`; a reader r finds predecessor p in the ring iff the kept rows in [p, r)
(p itself is one) number at most K and r - p <= 64; otherwise the row comes back from the stored matrix (far_row_reads).

THE WALK ON A PURE CHAIN (k_tracew, probe identical to the backbone): every round speculates min(VC_SPECW = 8, row, column) positions,
all confirm, and a general step would follow only a round that confirmed fewer than 8 without reaching (0, 0) -- on a chain of L rows
against L columns there is none.  chain_walk(L) = (L steps, L speculated, ceil(L / 8) rounds) per alignment.  Checked against the
definitions in include/vechat_hip.h (trace_steps: moves emitted; trace_spec: of which confirmed in bulk; trace_rounds: speculation
rounds -- a round that speculates nothing is not counted): case P_chain (chains of 200 and 203 rows, two alignments each) gives
806 / 806 / 102 in the linear overload with the kernels as they stood before this table existed, equal to 2 x (200 + 203) and
2 x (25 + 26); trace_steps equals the summed pair-list lengths of the oracle in every case (an alignment that leaves the band emits
nothing in its first walk and everything in its second).

Oracle time of the whole table (tests/test_trace_cases.py prints it): 2.8 s measured, budget ORACLE_BUDGET = 8 s (3 x).
"""
import functools

import numpy as np

import fwd_cases as fc
from fwd_cases import DEFAULT, cpl_for

VC_BAND_ROWS = 16
VC_BAND_LANES = 16
VC_TW_WIN = 256
VC_SPECW = 8
VC_INLINE_PRED = 6
VC_MAXTIE = 16
VC_KEPT = 6
ORACLE_BUDGET = 8.0


# ------------------------------------------------------------------------------------------------ restated geometry
def band_lanes(cpl):
    """vc_band_lanes (VC_BAND_CHAIN_COLS = 0)"""
    return 8 if cpl >= 10 else 10 if cpl >= 8 else 14 if cpl >= 6 else VC_BAND_LANES


def band_slope(length, nrows, cpl):
    """vc_band_slope: lanes per row, 16.16 fixed point"""
    return min(((length << 16) // nrows) // cpl, 0xFFFFFF)


def band_start(i, ql, bl):
    """vc_band_start; __umul24 keeps the low 32 bits of the product of the low 24 bits of each operand"""
    t = (((i & 0xFFFFFF) * (ql & 0xFFFFFF)) & 0xFFFFFFFF) >> 16
    return min(max(t, bl // 2 - 1) - (bl // 2 - 1), 64 - bl)


def band_row_start(r1, ql, bl):
    """vc_band_row_start; r1 = row - 1"""
    return band_start((r1 & ~(VC_BAND_ROWS - 1)) + 1 + VC_BAND_ROWS // 2, ql, bl)


class Band:
    """the stored band of one global alignment of `length` columns against `nrows` rows"""

    def __init__(self, length, nrows, cpl=None):
        self.cpl = cpl or cpl_for(length)
        self.bl = band_lanes(self.cpl)
        self.ql = band_slope(length, nrows, self.cpl)
        self.length, self.nrows = length, nrows
        self._start = [0] + [band_row_start(r - 1, self.ql, self.bl) for r in range(1, nrows + 1)]

    def start(self, r):
        return self._start[r]

    def in_band(self, r, c):
        if r == 0 or c == 0:
            return True
        return 0 <= (c - 1) // self.cpl - self._start[r] < self.bl


def banded(scores, cpl, nc):
    """vc_submit: bt->band = bt->packed && bt->kept"""
    return fc.row_packed(*scores.key(), cpl) and nc < 32768


def chain_walk(L):
    """k_tracew on a chain of L rows against L identical columns -> (steps, speculated, rounds)"""
    i = j = L
    spec = rounds = 0
    while i or j:
        f = min(VC_SPECW, i, j)
        assert f > 0                                          # (a general step would be needed: not on a chain)
        spec += f; rounds += 1; i -= f; j -= f
    return L, spec, rounds


# ------------------------------------------------------------------------------------------------ graphs and paths
def chain_graph(L, skips=()):
    """in-edge lists of rows 1 .. L (index 0 unused), in list order: the chain edge first, skip edges (from row, to row) in the order the
    layers add them (an edge that exists is not added again).  Row 1 has no in-edge: [] (the walk takes the virtual row 0)."""
    g = [[] for _ in range(L + 1)]
    for r in range(2, L + 1):
        g[r].append(r - 1)
    for a, b in skips:
        assert 1 <= a < b - 1 <= L - 1, (a, b)
        if a not in g[b]:
            g[b].append(a)
    return g


def skips_of(dels):
    """deleting backbone bases [a, a + d) (0-based) adds the edge row a -> row a + d + 1"""
    return [(a, a + d + 1) for a, d in dels]


def path(graph, backbone, probe, m, n, g):
    """int64 DP of `probe` against the graph over `backbone` (row r = backbone[r - 1]) and the reference's backtrack: diagonal through
    the in-edges in list order, then vertical through them in list order, then horizontal.  -> [(row, col)] from the end cell down to
    the cell before (0, 0), i.e. one cell per move."""
    a, b = np.frombuffer(backbone, np.uint8), np.frombuffer(probe, np.uint8)
    R, Cn = a.size, b.size
    j = np.arange(Cn + 1, dtype=np.int64)
    H = np.empty((R + 1, Cn + 1), np.int64)
    H[0] = j * g
    for r in range(1, R + 1):
        sc = np.where(b == a[r - 1], m, n).astype(np.int64)
        cur = np.full(Cn + 1, np.iinfo(np.int64).min // 2, np.int64)
        for pr in graph[r] or [0]:
            cur[1:] = np.maximum(cur[1:], np.maximum(H[pr, :-1] + sc, H[pr, 1:] + g))
            cur[0] = max(cur[0], H[pr, 0] + g)
        H[r] = np.maximum.accumulate(cur - j * g) + j * g
    r, c = R, Cn                                               # the only sink of a chain-plus-skip graph is its last row
    out = []
    while r or c:
        h = H[r, c]
        nxt = None
        preds = (graph[r] or [0]) if r else []
        if r and c:
            s = m if b[c - 1] == a[r - 1] else n
            nxt = next(((p, c - 1) for p in preds if h == H[p, c - 1] + s), None)
        if nxt is None and r:
            nxt = next(((p, c) for p in preds if h == H[p, c] + g), None)
        if nxt is None and c and h == H[r, c - 1] + g:
            nxt = (r, c - 1)
        assert nxt is not None
        out.append((r, c))
        r, c = nxt
    return out


def pairs_of(cells):
    """the oracle's pair list (node id or -1, sequence position or -1), first pair first, of a path() result on a chain-plus-skip graph"""
    out = []
    prev = (0, 0)
    for r, c in reversed(cells):
        out += [-1 if r == prev[0] else r - 1, -1 if c == prev[1] else c - 1]
        prev = (r, c)
    return out


def classify(graph, cells, band):
    """-> "outside" | "clear" | "unclear" (module docstring)"""
    if any(not band.in_band(r, c) for r, c in cells):
        return "outside"
    for r, c in cells:
        need = [(r, c - 1)] if c else []
        for pr in ((graph[r] or [0]) if r else []):
            need += [(pr, c)] + ([(pr, c - 1)] if c else [])
        if any(not band.in_band(x, y) for x, y in need):
            return "unclear"
    return "clear"


# ------------------------------------------------------------------------------------------------ windows
SPECIAL = bytes(c for c in range(66, 123) if chr(c).isalpha() and chr(c) not in "ACGTNacgtn")       # 42 letters outside ACGTN


def _backbone(rng, L, dels=(), distinct=()):
    """Backbone in which every deletion of the table has ONE optimal alignment.  With linear gaps a deleted block may be split and moved
    wherever the remaining bases still match, so the blocks are made of letters that occur nowhere else:
      dels:     blocks [a, a + d) that do not overlap: the block is drawn from G / T, everything else from A / C -- an alignment that
                matches every remaining base has to delete exactly the block;
      distinct: ranges [lo, hi) of at most 42 bases, each base a letter of its own (SPECIAL) -- any sub-block deleted from such a range
                (the common-end families F and N, single bases) is the only way to spell what remains."""
    bb = rng.choice(fc.ALPHA[:2] if dels else fc.ALPHA, L).astype(np.uint8)
    for a, d in dels:
        bb[a:a + d] = rng.choice(fc.ALPHA[2:], d)
    used = 0
    for lo, hi in distinct:
        assert used + hi - lo <= len(SPECIAL)
        bb[lo:hi] = np.frombuffer(SPECIAL[used:used + hi - lo], np.uint8)
        used += hi - lo
    return bb


def _qual(rng, n):
    return bytes(rng.integers(40, 70, n, dtype=np.uint8))


def _delete(bb, dels):
    keep = np.ones(bb.size, bool)
    for a, d in dels:
        keep[a:a + d] = False
    return bb[keep].tobytes()


class Win:
    """one window: backbone, a layer identical to it, deletion-only layers (dels: one list of (a, d) blocks per layer) and the probe"""

    def __init__(self, rng, bb, layer_dels, probe, tag="", identical=1):
        self.bb, self.tag, self.L = bb.tobytes(), tag, int(bb.size)
        self.layer_dels = [[]] * identical + [list(x) for x in layer_dels]
        self.layers = [_delete(bb, x) for x in self.layer_dels] + [probe]
        self.seqs = [self.bb] + self.layers
        self.quals = [_qual(rng, len(s)) for s in self.seqs]
        self.chain = True                                      # chain-plus-skip: paths are claimed

    def tuple(self):
        n = len(self.seqs)
        return (list(self.seqs), list(self.quals), [0] * n, [0] + [self.L - 1] * (n - 1))

    def graph_for(self, k):
        """the graph layer k (1-based; the probe is the last) is aligned to: the chain plus the skips of layers 1 .. k - 1"""
        sk = [s for x in self.layer_dels[:k - 1] for s in skips_of(x)]
        return chain_graph(self.L, sk)

    @functools.lru_cache(maxsize=None)
    def cells(self, k, scores=DEFAULT):
        return tuple(path(self.graph_for(k), self.bb, self.seqs[k], *scores.key()))

    @functools.lru_cache(maxsize=None)
    def klass(self, k, scores=DEFAULT):
        band = Band(len(self.seqs[k]), self.L)
        return classify(self.graph_for(k), self.cells(k, scores), band)


class TraceCase(fc.Case):
    """fwd_cases.Case with hand-ordered layers (presorted) and the claims of this table: exact (band_redo == outside alignments in the
    linear overload), far (None, or whether the build phase reads a row back from the stored matrix), chain (pure chains: counters)"""

    def __init__(self, name, hits, build, cpl, exact=False, far=None, chain=False, group=None, seed=0):
        super().__init__(name, hits, lambda rng: None, (cpl, cpl), (cpl, cpl), fc._form_default(cpl), group=group, seed=seed)
        self._wins, self.exact, self.far, self.chain = build, exact, far, chain

    @functools.lru_cache(maxsize=None)
    def wins(self):
        return tuple(self._wins(np.random.default_rng(self.seed)))

    @functools.lru_cache(maxsize=None)
    def windows(self):
        return [w.tuple() for w in self.wins()]

    @functools.lru_cache(maxsize=None)
    def batch(self):
        from vechat_amd import capi
        wins = self.windows()
        return capi.Batch.from_windows(wins, [0] * len(wins), presorted=True)

    def banded(self):
        return banded(self.scores, self.classes[1], self.nc())

    @functools.lru_cache(maxsize=None)
    def klasses(self):
        """classification of every build-phase alignment, window by window ([] when the launch is not banded: nothing can leave)"""
        if not self.banded():
            return tuple(() for _ in self.wins())
        return tuple(tuple(w.klass(k, self.scores) for k in range(1, len(w.seqs))) if w.chain else () for w in self.wins())

    def outside(self):
        return sum(k == "outside" for ks in self.klasses() for k in ks)


# ------------------------------------------------------------------------------------------------ family E: the band's edges per width
BAND_CLASSES = (4, 6, 8, 10, 16, 24)


def _probe_ins(bb, p, x):
    return bb[:p].tobytes() + x + bb[p:].tobytes()


def _search(make, lo, hi):
    """make(s) -> classification.  -> (s_in, s_out): the largest size that is clear and the smallest that is outside (a margin of unclear
    sizes lies between the two), by bisection; that both are monotone around the results is asserted"""
    a, b = lo, hi
    assert make(hi) == "outside" and make(lo) == "clear", (make(lo), make(hi))
    while b - a > 1:
        mid = (a + b) // 2
        a, b = (a, mid) if make(mid) == "outside" else (mid, b)
    s_out = b
    a, b = lo, s_out
    while b - a > 1:
        mid = (a + b) // 2
        a, b = (mid, b) if make(mid) == "clear" else (a, mid)
    s_in = a
    assert make(s_in) == "clear" and make(s_in + 1) != "clear" and make(s_out) == "outside" and make(s_out - 1) != "outside"
    return s_in, s_out


def _e_window(rng, cpl, kind, where):
    """-> {side: Win} for side in ("in", "out").  kind "ins": the probe is the backbone with a run of s random bases after row p, which
    pushes the path s columns to the right of the diagonal (L = 64 cpl - (bl + 1) cpl so that the longest probe stays in the class);
    kind "del": the probe lacks s bases behind row p, the path falls s columns to the left (L = 64 cpl).
      upper: p = cpl + 1 -- band_start is 0 there (left clamp): the band is lanes 0 .. bl - 1 whatever the slope
      cross: "ins": p = the multiple of 16 next to L / 2 -- the run lies on the last row of a band block, the diagonal behind it starts
             the next block; "del": p = 13 -- the vertical run crosses the block boundaries from row 16 on, and it starts near the top
             because the band follows the probe's own slope: behind a deletion at row p the path lies s (1 - (p + s) / L) columns left
             of the band's centre, which at p = L / 2 never reaches the edge
    The right clamp (band_start = 64 - bl) has no edge a path can cross: there the band ends at lane 63, beyond which no column exists,
    and its left edge lies further from the diagonal than anywhere else; an event in the last rows moves the path by s (1 - r / L)
    columns only, because the band follows the probe's own slope.  So no in / out pair exists there; _e_lower() adds a `clear` window
    whose path reads the clamped rows next to both of their ends."""
    bl = band_lanes(cpl)
    L = 64 * cpl - (bl + 1) * cpl if kind == "ins" else 64 * cpl
    mid = (L // 2) & ~15
    p = {"upper": cpl + 1, "cross": mid if kind == "ins" else 13}[where]
    hi = bl * cpl - 2
    seed = int(rng.integers(0, 1 << 30))

    def win(s, tag=""):
        r = np.random.default_rng(seed)
        if kind == "ins":                                      # a run of 'N' matches nothing: it is inserted whole, behind row p
            bb = _backbone(r, L)
            return Win(r, bb, [], bb[:p].tobytes() + b"N" * s + bb[p:].tobytes(), tag)
        bb = _backbone(r, L, [(p, s)])
        return Win(r, bb, [], _delete(bb, [(p, s)]), tag)

    @functools.lru_cache(maxsize=None)
    def make(s):
        return win(s).klass(2)
    s_in, s_out = _search(make, 2, hi)
    return {side: win(s, f"{kind} {where} p={p} s_{side}={s}") for side, s in (("in", s_in), ("out", s_out))}


def _e_lower(rng, cpl):
    """A `clear` alignment through the rows of the right clamp, L = 64 cpl: the probe lacks the s = (L - p) // 2 bases behind row
    p = (64 - bl) cpl + 2 and carries s bases 'N' at its end, so it keeps L columns and the slope stays 1.  The vertical run lies in
    column p, in the FIRST lane of the clamped band (the cells (r, p - 1) of the horizontal test are its first column); the run of 'N'
    lies on the last row up to column L, in lane 63.  A clamp that is off by a lane in the kernel loses one of the two: band_redo != 0.
    (Gapped 3 R - 8 s against shifted - R - 5 s with R = L - p - s bases of two letters behind the block: 4 R > 3 s.)"""
    bl = band_lanes(cpl)
    L = 64 * cpl
    p = (64 - bl) * cpl + 2
    s = (L - p) // 2
    bb = _backbone(rng, L, [(p, s)])
    return Win(rng, bb, [], _delete(bb, [(p, s)]) + b"N" * s, tag=f"del lower p={p} s={s} + {s} N: clear, in the clamped rows")


@functools.lru_cache(maxsize=None)
def _e_pair(cpl, kind):
    rng = np.random.default_rng(1000 + 10 * cpl + (kind == "del"))
    return [_e_window(rng, cpl, kind, where) for where in (("upper", "cross"))]


def _e(cpl, kind, side):
    return TraceCase(f"E{cpl}_{kind}_{side}", f"class {cpl}: a block {kind} of the largest clear size / the smallest size outside the band of "
                     f"{band_lanes(cpl)} lanes", lambda rng: [w[side] for w in _e_pair(cpl, kind)] + ([_e_lower(rng, cpl)] if (kind, side) == ("del", "in") else []),
                     cpl, exact=True, group=f"E{cpl}_{kind}", seed=cpl)


def _e32():
    """class 32: raw int16 rows under the shipped scores ((32 - 1) * 11 = 341 > 255): not banded, nothing can be redone (ACGT only: the
    lean form of the widest classes takes no other letter)"""
    def build(rng):
        L = 1792
        bb = _backbone(rng, L, [(896, 200)])
        return [Win(rng, bb, [], _probe_ins(bb, 896, rng.choice(fc.ALPHA, 200).tobytes()), tag="ins 200, raw rows"),
                Win(rng, bb, [], _delete(bb, [(896, 200)]), tag="del 200, raw rows")]
    return TraceCase("E32_raw", "class 32: raw rows, no band: a detour of 200 columns is not redone", build, 32, exact=True)


# ------------------------------------------------------------------------------------------------ family F: in-edge distances 15 / 16 / 17
def _f():
    """Node e + 1 (row e + 1) gets, behind its chain edge, skip edges of row distance 15, 16 and 17 (layers deleting the 14, 15, 16 bases in
    front of it).  The first in-edge of every row of a chain-plus-skip graph is the chain edge at distance 1, so the probes take these
    edges as a diagonal through in-edge 1, 2 and 3 of the general step, which reads 16-bit distances and has no bound at 15 / 16.  The
    limit of the 4-bit first-in-edge entry (vc_fie_entry: `d0 > 15` is not speculated) is NOT exercised by this table: it stays
    unpinned but for the string tripwire in test_restated_constants_are_those_of_the_sources."""
    def build(rng):
        L, e = 560, 300
        dels = [(e - d, d) for d in (14, 15, 16)]
        bb = _backbone(rng, L, distinct=[(e - 18, e + 2)])
        return [Win(rng, bb, [[x] for x in dels], _delete(bb, [x]), tag=f"probe deletes {x[1]}") for x in dels]
    return TraceCase("F15", "skip edges of row distance 15 / 16 / 17 into one node, each taken by a probe", build, 10, exact=True)


# ------------------------------------------------------------------------------------------------ family N: in-degree
IN_DEGREES = (3, 4, 6, 7, 9)


def _n(k):
    """Row e + 1 has in-degree k: the chain edge and skips of distance 2 .. k (layers deleting 1 .. k - 1 bases in front of it, in that
    order).  Probe A carries the longest deletion: a diagonal through the LAST in-edge (pass ceil(k / 3) of the general step; the
    VC_RF_OVF list beyond VC_INLINE_PRED = 6).  Probe B also lacks base e: the vertical move into row e + 1 through the last in-edge."""
    def build(rng):
        L, e = 200, 100
        dels = [(e - d, d) for d in range(1, k)]
        bb = _backbone(rng, L, distinct=[(e - k - 1, e + 2)])
        return [Win(rng, bb, [[x] for x in dels], _delete(bb, [dels[-1]]), tag="A: diagonal through the last in-edge"),
                Win(rng, bb, [[x] for x in dels], _delete(bb, [(e - k + 1, k)]), tag="B: vertical through the last in-edge")]
    return TraceCase(f"N{k}", f"in-degree {k}", build, 4, exact=True, group="N")


# ------------------------------------------------------------------------------------------------ family R: kept ring and far rows
def _r_dist(d):
    """one skip of row distance d (a layer deleting d - 1 bases); the probe is the backbone: its forward pass reads the predecessor from
    the ring (d <= 64) or from the stored matrix (d = 65)"""
    def build(rng):
        out = []
        for a in (60, 100):
            dels = [(a, d - 1)]
            bb = _backbone(rng, 200, dels)
            out.append(Win(rng, bb, [dels], bb.tobytes(), tag=f"distance {d} from row {a}"))
        return out
    return TraceCase(f"R_d{d}", f"read-back distance {d} of vc_frec_kept", build, 4, far=d > 64, group="R_d")


def _r_kept(nk):
    """a skip of row distance 40 from row p with nk kept rows in [p, r) (p itself and nk - 1 rows that skips of distance 2 read back);
    K = 6: nk = 6 finds p in the ring (kix[r] - kix[p] <= K), nk = 7 does not"""
    def build(rng):
        out = []
        for a in (60, 100):
            short = [(a + 4 + 5 * t, 1) for t in range(nk - 1)]      # rows a + 4 + 5 t are read back at distance 2
            bb = _backbone(rng, 200, [(a, 39)], distinct=[(x, x + 1) for x, _ in short])
            out.append(Win(rng, bb, [short, [(a, 39)]], bb.tobytes(), tag=f"{nk} kept rows behind row {a}"))
        return out
    return TraceCase(f"R_k{nk}", f"{nk} kept rows between reader and predecessor against K = {VC_KEPT}", build, 4, far=nk > VC_KEPT, group="R_k")


# ------------------------------------------------------------------------------------------------ family W: the sliding table window
JUMPS = (255, 256, 257, 320)


def _w_run():
    """the probe lacks 255 / 256 / 257 / 320 of 640 backbone bases behind row 20 and no layer has the skip edge: a vertical run through
    the chain, far outside the band; on whole rows (redo) the walk goes down row by row through general steps and k_tracew's window of
    VC_TW_WIN = 256 rows SLIDES with it (a block of 64 rows per round; the position never falls below the window).  s bases 'N' are
    appended so that the probe keeps 640 columns (class 10); with the deletion at row 20 the gapped alignment (3 (L - a - s) - 8 s)
    beats the shifted one (- (L - a - s) - 5 s)."""
    def build(rng):
        L, a = 640, 20
        out = []
        for s in JUMPS:
            bb = _backbone(rng, L, [(a, s)])
            out.append(Win(rng, bb, [], _delete(bb, [(a, s)]) + b"N" * s, tag=f"probe deletes {s}"))
        return out
    return TraceCase("W_run", "vertical runs of 255 .. 320 rows on whole rows: the table window slides along", build, 10, exact=True)


def _w_jump(cpl, L, sizes):
    """A layer deletes the s bases behind row 20, so row 20 + s + 1 has the skip edge from row 20 as its second in-edge, and the probe
    (the same sequence) takes it as a diagonal of the general step: the walk lands s + 1 rows lower in ONE step.  Coming down from the
    end cell the window has slid to 64 <= wlo <= position - 128 by then (it keeps fewer than 192 rows below the position), so row 20 lies below it:
    `gi < wlo` holds and win_init starts the window over.  Every sequence has to stay in one width class, and a class spans fewer
    than 512 columns: s = 255 .. 320 of 2 048 rows is class 32 (raw rows, no band: the first walk takes the jump; ACGT only), and
    s = 200 / 255 of 1 536 rows is class 24, where layer and probe are both `outside` and the jump is taken by the redo walk."""
    def build(rng):
        out = []
        for s in sizes:
            bb = _backbone(rng, L, [(20, s)])
            out.append(Win(rng, bb, [[(20, s)]], _delete(bb, [(20, s)]), tag=f"skip of {s + 1} rows taken by the probe"))
        return out
    return TraceCase(f"W_jump{cpl}", f"class {cpl}: a diagonal through a skip edge of {[s + 1 for s in sizes]} rows lands below the table window",
                     build, cpl, exact=True, group="W_jump")


def _w_rows(cpl, Ls):
    """backbones of nrows around a multiple of 64 (blk_store's mask of the last block): each probe has an inserted base in the first
    block of 64 rows and a deleted one in the last"""
    def build(rng):
        out = []
        for L in Ls:
            bb = _backbone(rng, L, distinct=[(L - 6, L - 5)])
            r = _delete(bb, [(L - 6, 1)])
            out.append(Win(rng, bb, [], r[:5] + b"N" + r[5:], tag=f"{L} rows"))
        return out
    return TraceCase(f"W_rows{cpl}", f"graphs of {Ls} rows", build, cpl, exact=True)


# ------------------------------------------------------------------------------------------------ family P: pure chains (counters)
def _p():
    def fix(rng):
        out = []
        for L in (200, 203):
            bb = _backbone(rng, L)
            out.append(Win(rng, bb, [], bb.tobytes(), tag=f"chain of {L}"))
        return out
    return TraceCase("P_chain", "probe identical to the backbone: trace_spec / trace_rounds of chain_walk()", fix, 4, exact=True, chain=True)


# ------------------------------------------------------------------------------------------------ family T: tied sinks
SINK_LETTERS = SPECIAL


class TieWin(Win):
    """nsinks - 1 layers identical to the backbone but for the last base, a letter of their own; the probe ends in yet another: every
    sink ties at the end cell.  The sinks' order is not unique: no path is claimed, only bytes and status."""

    def __init__(self, rng, L, nsinks):
        bb = _backbone(rng, L)
        self.bb, self.tag, self.L = bb.tobytes(), f"{nsinks} sinks", L
        self.layers = [self.bb[:-1] + SINK_LETTERS[k:k + 1] for k in range(nsinks)]       # the last one is the probe
        self.layer_dels = [[] for _ in self.layers]
        self.seqs = [self.bb] + self.layers
        self.quals = [_qual(rng, L) for _ in self.seqs]
        self.chain = False


def _t(nsinks):
    return TraceCase(f"T{nsinks}", f"{nsinks} sinks tied at the end cell (VC_MAXTIE = {VC_MAXTIE})", lambda rng: [TieWin(rng, 200, nsinks), TieWin(rng, 203, nsinks)], 4, group="T",
                     seed=nsinks)


SINKS = (15, 16, 17, 33)
E_CASES = [_e(c, kind, side) for c in BAND_CLASSES for kind in ("ins", "del") for side in ("in", "out")]
CASES = (E_CASES + [_e32(), _f()] + [_n(k) for k in IN_DEGREES] + [_r_dist(64), _r_dist(65), _r_kept(VC_KEPT), _r_kept(VC_KEPT + 1)] +
         [_w_run(), _w_jump(32, 2048, JUMPS), _w_jump(24, 1536, (200, 255)), _w_rows(4, (255, 256)), _w_rows(6, (257, 319, 320, 321)), _p()] + [_t(n) for n in SINKS])
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------ the oracle's view
@functools.lru_cache(maxsize=None)
def oracle_pairs(case, w, k):
    """(pair list, rank_to_node) of layer k of window w against the graph of the layers before it (vco_spoa_align_probe)"""
    import time
    import oracle_api as oa
    win = case.wins()[w]
    t0 = time.perf_counter()
    pairs, rank = oa.spoa_align_probe(oa.load_oracle(), "vco", list(win.seqs[:k]), list(win.quals[:k]), 1, *case.scores.key(), win.seqs[k], 1)
    fc.ORACLE_SECONDS[0] += time.perf_counter() - t0
    return tuple(pairs), tuple(rank)


def oracle_steps(case):
    """summed lengths of the build phase's pair lists: what trace_steps counts in the linear overload"""
    return sum(len(oracle_pairs(case, w, k)[0]) // 2 for w, win in enumerate(case.wins()) for k in range(1, len(win.seqs)))
