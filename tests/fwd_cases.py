"""TEST INFRASTRUCTURE: the case table of the forward pass's dispatch (tests/test_fwd_cases.py on the CPU, tests/test_fwd_classes_gpu.py
on the device).

The forward pass is a table of instantiations (launch_fwd / launch_fwd_t in vc_api.hip): 11 single width classes, 10 adjacent pairs,
the folded launch, each as k_fwd_dt, byte-packed k_fwd or raw k_fwd, with k_fwd_wide behind them.  Which one runs follows from
vc_cpl_for(len), vc_row_packed, vc_dt_ok and vc_int16_ok.  CASES below holds, for every instantiation and for every predicate's bound,
the smallest hand-built batch that reaches it: sequences of exactly 64 * CPL columns (every lane full), of 64 * CPL_prev + 1 (one
column in the class's first extra lane-column), batches that straddle a class edge by a single base, and score sets that sit on a
predicate's bound with their neighbour on the other side.  It also covers the 1 025 .. 2 048-column range (classes 20, 24 and 32) that
test_randomised_sweep_fixed_seed's list of lengths skips.

NOTHING THE LIBRARY EXPOSES TELLS A TEST WHICH INSTANTIATION RAN.  cpl_for, row_packed, dt_ok, int16_ok, nds, nc_for and route() are a
RESTATEMENT of the C predicates (vc_kernels.h, vc_fwd_dt.h) and of the host's decisions (vc_submit's bt->packed, maybe_wide and
capacity lines, launch_fwd's fold and dt lines), constants included; the routing the tests assert is this restatement.  Each C predicate
carries a comment naming this file: change the two together, and add the changed bound's edge cases to CASES.
"""
import functools
import time

import numpy as np

CLASSES = (4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64)
ALPHA = np.frombuffer(b"ACGT", np.uint8)
NC_MAX = 59968


# ------------------------------------------------------------------------------------------------ restated predicates
def cpl_for(length):
    """vc_cpl_for: the smallest instantiated width (columns per lane) that holds a sequence; 0 beyond 4 096 columns"""
    for c in CLASSES:
        if 64 * c >= length:
            return c
    return 0


def nds(cpl):
    """vc_nds: dwords per lane per row of the byte-packed stored form (cells + 16-bit anchor)"""
    return (cpl + 2 + 3) // 4


def spread_bound(m, n, g, cpl):
    """what vc_row_packed compares with 255: the largest difference between a lane's first cell and any of its cells"""
    return (cpl - 1) * (max(m, n) - 2 * g)


def row_packed(m, n, g, cpl):
    """vc_row_packed"""
    return g < 0 and spread_bound(m, n, g, cpl) <= 255


def dt_top(m, g, nrows, cpl):
    """what vc_dt_ok compares with 65 000"""
    return max(m, 0) * (64 * cpl + 1) + (nrows + 64 * cpl + 1 + 8) * (-g)


def dt_ok(m, n, g, nrows, cpl):
    """vc_dt_ok"""
    if g >= 0 or n - 2 * g < 0 or m - 2 * g < 0:
        return False
    return dt_top(m, g, nrows, cpl) <= 65000 and row_packed(m, n, g, cpl)


def int16_cols(m, g, cpl):
    """what vc_int16_ok compares with 32 767"""
    return (m - g) * (64 * cpl + 1)


def int16_ok(m, n, g, nrows, cpl, nw):
    """vc_int16_ok"""
    if g >= 0 or (not nw and n >= 0):
        return False
    dec = max(-g, -(n - g))
    lo = -(nrows + 8) * dec if nw else 0
    return lo >= -31744 and int16_cols(m, g, cpl) < 32767


def nc_for(windows, max_nodes=0):
    """vc_submit's row capacity of a cold context for a batch: windows = [(backbone length, [layer lengths])]"""
    if max_nodes:
        return (max_nodes + 63) & ~63
    need = 0
    for L, lens in windows:
        d = len(lens)
        est = 0.33 * (sum(lens) / d) * d ** 0.55 if d else 0.0
        need = max(need, L + int(np.ceil(est)) + 64)
    return min((min(need, NC_MAX) + 63) & ~63, NC_MAX)


def route(params, NC, cpl_min, cpl, vc_dt=True, pure=True):
    """-> (instantiation, form, wide_behind) as launch_fwd and vc_submit decide them for a batch whose shortest / longest sequence fall in
    classes cpl_min / cpl, on workspaces of NC rows.
    instantiation: (CA, CB) as in launch_fwd_t<CA, CB>; a folded launch (more than two classes) is ("fold", CB_prev, CB).
    form: "dt"        global alignments on k_fwd_dt, local ones on byte-packed k_fwd;
          "packed"    k_fwd on byte-packed rows;
          "raw"       k_fwd on int16 pairs;
          "wide-only" the packed-int16 kernel declines every alignment of the top class (column bound of vc_int16_ok, or a class of 32+
                      columns per lane without the lean form): k_fwd_wide computes them.
    wide_behind: k_fwd_wide is launched behind the packed-int16 kernel (maybe_wide).
    params: anything with match / mismatch / gap / sw_match / sw_mismatch / sw_gap."""
    m, n, g = params.match, params.mismatch, params.gap
    sm, sn, sg = params.sw_match, params.sw_mismatch, params.sw_gap
    lo, hi = CLASSES.index(cpl_min), CLASSES.index(cpl)
    inst = (cpl, cpl) if lo == hi else (CLASSES[hi - 1], cpl) if hi - lo == 1 else ("fold", CLASSES[hi - 1], cpl)
    packed = row_packed(m, n, g, cpl) and row_packed(sm, sn, sg, cpl)
    lean = (1 if pure and n - g == -1 else 0) | (2 if pure and sn - sg == -1 else 0)
    wide = not int16_ok(m, n, g, NC, cpl, True) or not int16_ok(sm, sn, sg, NC, cpl, False) or (cpl >= 32 and lean != 3)
    declined = int16_cols(m, g, cpl) >= 32767 or int16_cols(sm, sg, cpl) >= 32767 or g >= 0 or sg >= 0 or sn >= 0 or (cpl >= 32 and lean != 3)
    dt = vc_dt and packed and cpl < 32 and dt_ok(m, n, g, NC, cpl)
    form = "wide-only" if declined else "dt" if dt else "packed" if packed else "raw"
    return inst, form, wide


# ------------------------------------------------------------------------------------------------ case builder
def _fit(rng, r, n, alpha=ALPHA):
    """random single-base deletions or insertions until r has exactly n bases"""
    r = list(r)
    while len(r) > n:
        del r[int(rng.integers(0, len(r)))]
    while len(r) < n:
        r.insert(int(rng.integers(0, len(r) + 1)), int(rng.choice(alpha)))
    return bytes(r)


def _read(rng, src, n, sub, events=(), alpha=ALPHA):
    r = src.copy()
    mut = rng.random(r.size) < sub
    r[mut] = rng.choice(alpha, int(mut.sum()))
    r = r.tobytes()
    for kind, pos, size in events:
        assert size >= 30
        r = r[:pos] + (rng.choice(alpha, size).tobytes() + r[pos:] if kind == "ins" else r[pos + size:])
    r = _fit(rng, r, n, alpha)
    return r, bytes(rng.integers(40, 70, n, dtype=np.uint8))


def window(rng, L, lens, sub=0.05, events=(), alpha=ALPHA):
    """A hand-built window: random ACGT backbone of L bases with quality, one full-span layer per entry of lens of exactly that length
    (substitutions at rate sub, then random deletions / insertions to hit the length, random qualities).
    events: (layer, "ins" | "del", position, size >= 30) -- a block insertion / deletion in that layer (layers count from 1): a lane then
    holds a vertical-then-horizontal detour next to a diagonal run.  -> (seqs, quals, begins, ends) for capi.Batch.from_windows"""
    bb = rng.choice(alpha, L)
    seqs, quals, b, e = [bb.tobytes()], [bytes(rng.integers(40, 70, L, dtype=np.uint8))], [0], [0]
    for k, n in enumerate(lens, 1):
        r, q = _read(rng, bb, n, sub, [ev[1:] for ev in events if ev[0] == k], alpha)
        seqs.append(r); quals.append(q); b.append(0); e.append(L - 1)
    return seqs, quals, b, e


def piece(rng, win, begin, end, n, sub=0.05):
    """Adds a partial-span layer of exactly n bases to a window(): backbone[begin .. end] with substitutions at rate sub, fitted to n.
    sub=None: the first n bases of the backbone, unchanged (begin / end are then only the layer's claimed position)."""
    seqs, quals, b, e = win
    L = len(seqs[0])
    off = int(0.01 * L)
    assert not (begin < off and end > L - off) and begin < end < L, "a piece must not span the window"
    bb = np.frombuffer(seqs[0], np.uint8)
    if sub is None:
        r, q = bb[:n].tobytes(), bytes(rng.integers(40, 70, n, dtype=np.uint8))
        assert len(r) == n
    else:
        r, q = _read(rng, bb[begin:end + 1], n, sub)
    seqs.append(r); quals.append(q); b.append(begin); e.append(end)
    return win


def full_span(begin, end, L):
    """vc_full_span (window.cpp:212, 253-254): such a layer is aligned globally, any other locally"""
    off = int(0.01 * L)
    return begin < off and end > L - off


def lens_of(win):
    return len(win[0][0]), [len(s) for s in win[0][1:]]


class Scores:
    def __init__(self, m, n, g):
        self.match = self.sw_match = m
        self.mismatch = self.sw_mismatch = n
        self.gap = self.sw_gap = g

    def kw(self):
        return dict(match=self.match, mismatch=self.mismatch, gap=self.gap, sw_match=self.match, sw_mismatch=self.mismatch, sw_gap=self.gap)

    def key(self):
        return (self.match, self.mismatch, self.gap)


DEFAULT = Scores(3, -5, -4)          # capi.default_params(): max(m, n) - 2g = 11, mismatch - gap = -1 (the lean form's condition)


class Case:
    """name; hits: what the case is there for; build(rng) -> windows; scores; max_nodes (0: the host's estimate);
    classes: (cpl_min, cpl) claimed; inst / form: the claimed routing; group: cases that are one pair split by a predicate"""

    def __init__(self, name, hits, build, classes, inst, form, scores=DEFAULT, max_nodes=0, max_edges=0, group=None, seed=0, probe=1):
        self.name, self.hits, self._build, self.classes, self.inst, self.form = name, hits, build, classes, inst, form
        self.scores, self.max_nodes, self.max_edges, self.group, self.seed, self.probe = scores, max_nodes, max_edges, group, seed, probe

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def windows(self):
        return self._build(np.random.default_rng(self.seed))

    @functools.lru_cache(maxsize=None)
    def batch(self):
        from vechat_amd import capi
        wins = self.windows()
        return capi.Batch.from_windows(wins, [0] * len(wins))

    def params(self, mode=0, **kw):
        from vechat_amd import capi
        return capi.default_params(mode=mode, max_nodes=self.max_nodes, max_edges=self.max_edges, **self.scores.kw(), **kw)

    def seq_classes(self):
        return sorted({cpl_for(len(s)) for w in self.windows() for s in w[0]})

    def pure(self):
        return all(set(q) <= set(b"ACGT") for w in self.windows() for q in w[0])

    def route(self, NC=None, vc_dt=True):
        return route(self.scores, self.nc() if NC is None else NC, *self.classes, vc_dt=vc_dt, pure=self.pure())

    def nc(self):
        return nc_for([lens_of(w) for w in self.windows()], self.max_nodes)


ORACLE_SECONDS = [0.0]


@functools.lru_cache(maxsize=None)
def oracle(case, mode):
    """(consensus bytes per window, polished flags, stats) of a case in one overload: computed once, shared, never changed"""
    import oracle_api as oa
    t0 = time.perf_counter()
    ref, pol, st = oa.oracle_run(case.batch(), case.params(mode))
    ORACLE_SECONDS[0] += time.perf_counter() - t0
    return tuple(ref), tuple(int(p) for p in pol), dict(cells=int(st.cells), max_nodes=int(st.max_nodes), max_edges=int(st.max_edges))


# ------------------------------------------------------------------------------------------------ the table
def _prev(cpl):
    i = CLASSES.index(cpl)
    return CLASSES[i - 1] if i else 0


def _form_default(cpl):
    # D4: under the shipped scores class 24 is the last byte-packed, banded, k_fwd_dt class ((24 - 1) * 11 = 253 <= 255) and class 32 the
    # first that exists in the lean / raw form only: A24 against A32 (and B24_32, C24_32) is the packed/dt <-> raw boundary of the defaults
    return "dt" if cpl <= 24 else "raw"


def _a(cpl):
    top, lo = 64 * cpl, 64 * _prev(cpl) + 1

    def build(rng):
        return [window(rng, top - 3, [top, top - 1, top, top - 7, top - 2]),             # "top": every lane full, last lane masks
                window(rng, lo + 2, [lo, lo + 1, lo + 3, lo])]                           # "bottom": one column in the first extra lane-column
    return Case(f"A{cpl}", f"k_fwd<{cpl},{cpl}> alone: reads of exactly {top} columns and of {lo}", build, (cpl, cpl), (cpl, cpl),
                _form_default(cpl), seed=100 + cpl)


def _b(ca, cb):
    e = 64 * ca
    nl = 5

    def build(rng):
        return [window(rng, e - 1, [e - 1, e, e + 1, e + 2, e][:nl]),       # straddles the edge by one or two columns
                window(rng, e - 5, [e - 2, e, e - 9, e - 1][:nl])]                                       # entirely in CA: narrower jobs in the CA half of the launch
    return Case(f"B{ca}_{cb}", f"k_fwd<{ca},{cb}>: a window straddling {e} columns by one or two, beside one entirely in class {ca}",
                build, (ca, cb), (ca, cb), _form_default(cb), seed=200 + cb)


def _c(ca, cb):
    a, b = 64 * ca, 64 * cb

    def build(rng):
        w0 = window(rng, a - 10, [a - 1, a, a - 20])
        for n, at in ((100, 40), (300, a // 3), (700, a // 4)):
            piece(rng, w0, at, at + n - 1 + 6, n)
        w1 = window(rng, b - 30, [b, b - 1, b - 40])
        for n, at in ((700, 100), (100, b // 2), (300, b - 400)):
            piece(rng, w1, at, at + n - 1 - 5, n)
        return [w0, w1]
    return Case(f"C{ca}_{cb}", f"folded launch over classes {ca}/{cb} with partial-span pieces of 100, 300 and 700 columns in its lower half",
                build, (cpl_for(100), cb), ("fold", ca, cb), _form_default(cb), seed=300 + cb)


def _d255(cpl, g, n=-4):
    """vc_row_packed at exactly 255 (m = 5) against just above (m = 6); layers carry block insertions / deletions"""
    top, lo = 64 * cpl, 64 * _prev(cpl) + 1
    span = top - lo

    def build(rng):
        ev = [(1, "ins", lo // 2 + 3, 32), (2, "del", lo // 3 + 1, 31), (3, "ins", lo // 4, 30)] if lo > 100 else \
             [(1, "ins", 60, 32), (2, "del", 90, 31), (3, "ins", 120, 30)]
        return [window(rng, top - 3, [top, top - 1, top - 5, top - 2], events=ev),
                window(rng, lo + span // 2, [lo + 1, top, lo + span // 3, lo + span // 2], events=ev[:2])]
    out = []
    for m in (5, 6):
        s = Scores(m, n, g)
        out.append(Case(f"D255_c{cpl}_m{m}", f"vc_row_packed at class {cpl}: spread bound {spread_bound(m, n, g, cpl)} "
                        f"({'byte-packed' if m == 5 else 'raw int16 pairs'})", build, (cpl, cpl), (cpl, cpl), "dt" if m == 5 else "raw",
                        scores=s, max_nodes=768 if cpl == 4 else 0, group=f"D255_c{cpl}", seed=400 + cpl))
    return out


# vc_dt_ok at 65 000: m = 4, n = -6, g = -16 at class 8 holds up to 3 413 rows (4 * 513 + (NC + 521) * 16 <= 65 000); capacities are
# multiples of 64, so 3 392 rows is the last capacity on the dt side and 3 456 the first beyond it.
DT_SCORES = Scores(4, -6, -16)
DT_NC = (3392, 3456)
DT_DEPTH = 48             # layers of the window, found on the CPU: see DT_ROWS
DT_SUB = 0.3
DT_ALPHA = np.frombuffer(b"ACGTRYKM", np.uint8)
# With g = -16 against n = -6 a read is aligned through mismatches, not gaps: the graph gains letters per column, hardly any columns,
# and four letters saturate near 2 400 rows however deep the window is.  Eight letters reach the capacity.
# Rows of the oracle's graph at the end of the build (the largest graph the forward pass meets; the prunes of the haplotype overload
# shrink it afterwards), found with oracle_run's max_nodes / oracle_stages; test_fwd_cases.py asserts DT_ROWS and 0.9 * 3 392 <= DT_ROWS <= 3 392.
DT_ROWS = 3365


def _ddt():
    def build(rng):
        rs = np.random.default_rng(77)
        lens = [int(x) for x in rs.integers(400, 513, DT_DEPTH)]
        return [window(rng, 500, lens, sub=DT_SUB, alpha=DT_ALPHA), window(rng, 450, [400, 512, 385, 470])]
    return [Case(f"Ddt_nc{nc}", f"vc_dt_ok at class 8, capacity {nc}: top cell bound {dt_top(4, -16, nc, 8)} against 65 000", build, (8, 8), (8, 8),
                 "dt" if nc == DT_NC[0] else "packed", scores=DT_SCORES, max_nodes=nc, max_edges=16000, group="Ddt", seed=500) for nc in DT_NC]


def _d16():
    """vc_int16_ok's column bound at class 4: (m - g) * 257 = 32 639 < 32 767 (k_fwd, raw rows) against 32 896 (k_fwd_wide).  Layer 1 is a
    partial-span piece identical to the 256 backbone bases: its local alignment's tilted score reaches (m - g) * 256.  The capacity is
    pinned to 448 rows: (448 + 8) * 67 = 30 552 <= 31 744, so the global rows stay inside int16 with dec = 67 and no k_fwd_wide is planned."""
    def build(rng):
        w0 = window(rng, 256, [])
        piece(rng, w0, 3, 250, 256, sub=None)
        for n in (256, 250, 255):
            r, q = _read(rng, np.frombuffer(w0[0][0], np.uint8), n, 0.03)
            w0[0].append(r); w0[1].append(q); w0[2].append(0); w0[3].append(255)
        return [w0, window(rng, 200, [193, 256, 230], sub=0.03)]
    out = []
    for m in (60, 61):
        out.append(Case(f"D16_m{m}", f"vc_int16_ok's column bound at class 4: (m - g) * 257 = {int16_cols(m, -67, 4)} against 32 767", build, (4, 4), (4, 4),
                        "raw" if m == 60 else "wide-only", scores=Scores(m, -10, -67), max_nodes=448, max_edges=2048, group="D16", seed=600))
    return out


PAIRS = tuple((CLASSES[i], CLASSES[i + 1]) for i in range(10))
# Order matters to the device test: one warm context sees classes 4 -> 64 (A), the pairs (B), the folds (C), and then class 8 again.
CASES = ([_a(c) for c in CLASSES] + [_b(a, b) for a, b in PAIRS] + [_c(20, 24), _c(24, 32), _c(48, 64)] +
         _d255(16, -6) + _d255(6, -23) + _d255(4, -40) + _ddt() + _d16())
BY_NAME = {c.name: c for c in CASES}

# Attained on the CPU (tests/test_fwd_cases.py::test_envelope_attainment prints this table; layer 1 against the backbone only --
# attainment in later layers, against a branching graph, is not computed on the CPU):
#   case           bound that claims it            attained on layer 1
ATTAINED = {
    'D255_c16_m5'                 : (255, 16665, -6126, 10539),            # global
    'D255_c16_m6'                 : (270, 17634, -6126, 11508),            # global
    'D255_c6_m5'                  : (255, 18027, -8763, 9264),             # global
    'D255_c6_m6'                  : (260, 18350, -8763, 9587),             # global
    'D255_c4_m5'                  : (255, 20170, -10120, 10094),           # global
    'D255_c4_m6'                  : (258, 20300, -10120, 10220),           # global
    'Ddt_nc3392'                  : (252, 13706, -8000, 5708),             # global
    'Ddt_nc3456'                  : (252, 13706, -8000, 5708),             # global
    'D16_m60'                     : (582, 0, 0, 32512),                    # local
    'D16_m61'                     : (585, 0, 0, 32768),                    # local
    'D16_m60 (layer 2, global)'   : (582, 49454, -17152, 32302),           # global
}


# ------------------------------------------------------------------------------------------------ plain DP of one layer against the backbone
def tilted_extremes(backbone, read, m, n, g, cpl, local):
    """int64 DP of `read` (columns) against the chain graph of `backbone` (rows), global or local, in the forward kernels' three forms:
    -> dict(spread: largest T[last cell of a lane] - T[first cell of that lane] over all rows (T = H - j*g; bound 255),
            t2_max: largest T'' = H - (i + j)*g (global only; bound 65 535), t_min / t_max: extremes of T (bounds -31 744 / 32 767))"""
    a = np.frombuffer(backbone, np.uint8)
    b = np.frombuffer(read, np.uint8)
    R, Cn = a.size, b.size
    j = np.arange(Cn + 1, dtype=np.int64)
    prev = np.zeros(Cn + 1, np.int64) if local else j * g
    first = np.arange(0, Cn, cpl) + 1                      # lane l owns columns l * cpl + 1 .. (l + 1) * cpl
    last = np.minimum(first + cpl - 1, Cn)
    out = dict(spread=0, t2_max=0, t_min=0, t_max=0)
    for i in range(1, R + 1):
        sc = np.where(b == a[i - 1], m, n).astype(np.int64)
        cur = np.empty(Cn + 1, np.int64)
        cur[0] = 0 if local else i * g
        cur[1:] = np.maximum(prev[:-1] + sc, prev[1:] + g)
        if local:
            cur[1:] = np.maximum(cur[1:], 0)
        # horizontal moves: H[j] = max(H[j], H[j-1] + g)  <=>  prefix maximum of T = H - j*g
        T = np.maximum.accumulate(cur - j * g)
        cur = T + j * g
        out["spread"] = max(out["spread"], int((T[last] - T[first]).max()))
        out["t_min"] = min(out["t_min"], int(T.min())); out["t_max"] = max(out["t_max"], int(T.max()))
        if not local:
            out["t2_max"] = max(out["t2_max"], int((T - i * g).max()))
        prev = cur
    return out
