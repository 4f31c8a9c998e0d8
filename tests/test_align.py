"""GPU suite for the overlap aligner.  Parity with edlib cannot be pinned (not vendored, and an
optimal path is not unique).  What is pinned is the aligner's own promise (header of vechat_amd/csrc/vc_align.hip): the optimal path
chosen from the end by diagonal, then insertion, then deletion.  tests/align_ref.py restates that on the CPU with the full matrix, and
every pair a test below submits is compared with it by CIGAR string, byte for byte, and by distance -- a path crosses every row and
every column and the traceback decodes three neighbours per step, so every lane and slot of the packed storage is read on the way.
The first test is the older, weaker statement (a valid global alignment whose cost is the edit distance) at the largest shapes.
The chunk loop and the envelope run under the knobs VC_ALIGN_BUDGET_MB / VC_ALIGN_MAX_MAT_MB, proven by the VC_ALIGN_LOG lines."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import align_ref

pytestmark = pytest.mark.gpu


def edit_distance(q, t):
    qa, ta = np.frombuffer(q, np.uint8), np.frombuffer(t, np.uint8)
    m = len(t)
    idx = np.arange(m + 1)
    row = idx.astype(np.int64)
    for i in range(1, len(q) + 1):
        new = np.empty(m + 1, np.int64)
        new[0] = i
        if m:
            new[1:] = np.minimum(row[:-1] + (ta != qa[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(new - idx) + idx
    return int(row[m])


def cigar_cost(cigar, q, t):
    """walks the CIGAR over both sequences; returns its cost, or None if it does not consume them exactly"""
    i = j = cost = 0
    for num, op in re.findall(r"(\d+)([MID])", cigar):
        n = int(num)
        if op == "M":
            if i + n > len(q) or j + n > len(t):
                return None
            cost += sum(1 for k in range(n) if q[i + k] != t[j + k]); i += n; j += n
        elif op == "I":
            cost += n; i += n
        else:
            cost += n; j += n
    return cost if (i, j) == (len(q), len(t)) and re.fullmatch(r"(\d+[MID])*", cigar) else None


def _mut(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate * 0.3:
            continue
        if r < rate * 0.7:
            out.append(rng.choice(b"ACGT"))
        out.append(rng.choice(b"ACGT") if rate * 0.7 <= r < rate else c)
    return bytes(out)


def test_cigars_are_optimal_global_alignments(built):
    from vechat_amd.align import align_pairs
    rng = random.Random(11)
    pairs = [(b"A", b"A"), (b"A", b"C"), (b"ACGT", b"A"), (b"A", b"ACGTACGT"), (b"ACGTTGCA", b"ACGTTGCA"),
             (b"", b"ACG"), (b"ACG", b""), (b"", b"")]
    for L in (7, 33, 64, 65, 500, 2047, 2048, 2049, 3000, 4500):
        t = bytes(rng.choice(b"ACGT") for _ in range(L))
        pairs.append((_mut(rng, t, 0.25) or b"A", t))
        pairs.append((t, _mut(rng, t, 0.1) or b"A"))
    pairs.append((bytes(rng.choice(b"ACGT") for _ in range(300)), bytes(rng.choice(b"ACGT") for _ in range(2500))))   # unrelated
    pairs.append((b"ACGTNNACGT" * 30, b"ACGTACGT" * 40))
    rng2 = random.Random(5)
    long_t = bytes(rng2.choice(b"ACGT") for _ in range(21000))                # beyond int16 as an absolute score: relative scores
    long_q = _mut(rng2, long_t, 0.2)
    cg_big, d_big = align_pairs([pairs[0], (long_q, long_t), pairs[1]])
    assert d_big[0] == 0 and d_big[2] == 1 and cg_big[0] == "1M"
    assert d_big[1] == edit_distance(long_q, long_t) and cigar_cost(cg_big[1], long_q, long_t) == d_big[1]
    cigars, dist = align_pairs(pairs)
    for (q, t), cg, d in zip(pairs, cigars, dist):
        assert d == edit_distance(q, t), (len(q), len(t))
        assert cigar_cost(cg, q, t) == d, (len(q), len(t), cg[:60])


@pytest.mark.parametrize("dist_path", [False, True])
def test_paf_without_cigar_end_to_end(built, tmp_path, capsys, monkeypatch, dist_path):
    """The VeChat driver's own input shape: PAF from minimap2 without cg tags.  The command line aligns the
    overlaps on the device first; the corrected reads must come out polished and close to the truth."""
    import fixtures
    from test_seqio import write_inputs
    from vechat_amd import polish
    if dist_path:                                   # one-process-per-GPU path (sharded alignment, RCCL exchange), single rank
        monkeypatch.setenv("VC_FORCE_DIST", "1")
        monkeypatch.setenv("MASTER_PORT", "29549")
    fx, wb = fixtures.load_plumbing()
    wb.close()
    rp, op, tp = write_inputs(fx, tmp_path, sam=False)
    txt = "\n".join(ln.split("\tcg:Z:")[0] for ln in open(op).read().strip().split("\n")) + "\n"
    open(op, "w").write(txt)
    assert polish.main([str(rp), str(op), str(tp), "-p", "-d", "0.2", "-s", "0.2"]) == 0
    out = capsys.readouterr().out.strip().split("\n")
    got = {out[i][1:].split()[0]: out[i + 1] for i in range(0, len(out), 2)}
    exp = {n.split()[0]: d for n, d in fx["expected"]["hap"]["stitched"]}
    assert set(got) == set(exp)
    for name in exp:                       # another optimal alignment moves a few window boundaries: near-identical, not identical
        assert abs(len(got[name]) - len(exp[name])) < 0.05 * len(exp[name])
        assert edit_distance(got[name].encode(), exp[name].encode()) < 0.05 * len(exp[name])


# ---------------------------------------------------------------------------------------------------------------------------
# The path itself, against tests/align_ref.py.  Every pair of every call is compared; references are computed once per pair.
_REF = {}
_KNOBS = ("VC_ALIGN_BUDGET_MB", "VC_ALIGN_MAX_MAT_MB", "VC_ALIGN_LOG")


def _ref(q, t):
    if (q, t) not in _REF:
        _REF[(q, t)] = align_ref.align(q, t)
    return _REF[(q, t)]


def _compare(pairs, cigars, dist, except_for=()):
    assert len(cigars) == len(dist) == len(pairs)
    for k, (q, t) in enumerate(pairs):
        if k in except_for:
            continue
        cg, d = _ref(q, t)
        assert dist[k] == d, (k, len(q), len(t), dist[k], d)
        assert cigars[k] == cg, (k, len(q), len(t), cigars[k][:80], cg[:80])


def _check(pairs):
    from vechat_amd.align import align_pairs
    cigars, dist = align_pairs(pairs)
    _compare(pairs, cigars, dist)
    return cigars, dist


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _mut_to(rng, s, n, rate=0.15):
    """s with substitutions, insertions and deletions, then cut or filled up at the end to exactly n bases"""
    out = _mut(rng, s, rate)[:n]
    return out + _rand(rng, n - len(out))


def _slice_of(rng, t, n, rate=0.15):
    """a mutated piece of t of exactly n bases taken from t's middle: the optimal path leaves the matrix edges"""
    lo = max(0, (len(t) - n) // 2)
    return _mut_to(rng, t[lo:lo + n], n, rate)


KNOWN = [(b"AAA", b"AAAAA", "2D3M", 2), (b"AAAAA", b"AAA", "2I3M", 2), (b"AAA", b"CCCCC", "2D3M", 5), (b"ACGT", b"A", "1M3I", 3),
         (b"A", b"ACGTACGT", "4D1M3D", 7), (b"ACAC", b"AC", "2I2M", 2), (b"AC", b"ACAC", "2D2M", 2), (b"AG", b"GA", "2M", 2),
         (b"ACGT", b"AGT", "1M1I2M", 1), (b"", b"ACG", "3D", 3), (b"ACG", b"", "3I", 3), (b"", b"", "", 0)]


def test_known_answers_on_the_device(built):
    """the hand-derived table of tests/test_align_ref.py, as one call"""
    pairs = [(q, t) for q, t, _, _ in KNOWN]
    cigars, dist = _check(pairs)
    assert cigars == [cg for _, _, cg, _ in KNOWN] and dist == [d for _, _, _, d in KNOWN]


ROWS = (1, 63, 64, 65, 127, 128, 129)                        # k_aln_fwd walks the query in blocks of 64 rows
COLS = (1, 31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097)   # a lane holds 32 columns, a tile 2048


@pytest.mark.parametrize("related", [False, True], ids=["unrelated", "slice"])
def test_row_block_edges_times_tile_edges(built, related):
    """every n at a row-block edge with every m at a lane or tile edge, one call per case: unrelated sequences, and q a mutated slice
    from the middle of t (the path runs through the interior, long diagonals)"""
    rng = random.Random(101 + related)
    pairs = []
    for n in ROWS:
        for m in COLS:
            t = _rand(rng, m)
            pairs.append((_slice_of(rng, t, n) if related else _rand(rng, n), t))
    assert sorted({(len(q), len(t)) for q, t in pairs}) == sorted((n, m) for n in ROWS for m in COLS)
    _check(pairs)


def test_paths_along_the_matrix_edges(built):
    """n >> m and m >> n: the path runs down a side of the matrix, the boundary difference stays at +-1 for thousands of rows"""
    rng = random.Random(102)
    pairs = []
    for n, m in ((5000, 1), (5000, 3), (1, 5000), (3, 5000)):
        pairs.append((_rand(rng, n), _rand(rng, m)))
        long = _rand(rng, max(n, m)); short = long[2500:2500 + min(n, m)]           # the short one occurs in the long one
        pairs.append((long, short) if n > m else (short, long))
    long = _rand(rng, 3000)
    for lo in (0, 1450, 2900):                                                       # embedded at the start, the middle, the end
        for short in (long[lo:lo + 100], _mut_to(rng, long[lo:lo + 100], 100)):
            pairs.append((long, short))
            pairs.append((short, long))
    _check(pairs)


def test_boundary_columns_beyond_int16(built):
    """130 x 40 000: 20 tiles, boundary values down to -38 912, which only the int32 boundary columns hold.  q from the far end of t
    (the path hugs row 0 for 39 800 columns), q unrelated, and the tall case 40 000 x 130 (one tile, 625 row blocks)."""
    rng = random.Random(103)
    t = _rand(rng, 40000)
    pairs = [(_mut_to(rng, t[39800:39930], 130), t), (_rand(rng, 130), t), (t, _mut_to(rng, t[20000:20130], 130))]
    _check(pairs)
    D = align_ref.matrix(pairs[1][0], t)
    assert int(D[0, 19 * 2048]) == 38912 and int(D[:, 17 * 2048].min()) > 32767        # whole boundary columns beyond int16


def test_maximal_ties(built):
    """homopolymers, all-mismatch, dinucleotide repeats in and out of phase: nearly every cell has co-optimal predecessors, so
    only the tie-break order decides the path"""
    shapes = ((64, 2049), (2049, 64), (200, 200), (65, 4097))
    pairs = [(b"A" * k, b"A" * m) for k, m in shapes]
    pairs += [(b"A" * k, b"C" * m) for k, m in shapes]
    for a, b in ((32, 1025), (1025, 32), (100, 100), (65, 2049)):
        pairs += [(b"AC" * a, b"AC" * b), (b"AC" * a, b"CA" * b)]
    pairs.append((b"ACGTNNACGT" * 30, b"ACGTACGT" * 40))
    _check(pairs)


def test_bytes_outside_acgt(built):
    """any byte is a base and equals only itself -- 0xFF too, the value the forward kernel pads the columns >= m with"""
    rng = random.Random(104)
    every = bytes(range(256))
    pairs = []
    for n, m in ((129, 2049), (64, 33)):
        t = _rand(rng, m, every)
        pairs += [(_rand(rng, n, every), t), (bytes(rng.choice(every) if rng.random() < 0.2 else c for c in t[m // 3:m // 3 + n]), t)]
    for m in (33, 2047, 4097):                                   # odd m: the last packed pair of columns is half padding
        pairs.append((b"\xff" * 70, _rand(rng, m, b"\xffA")))
        pairs.append((b"\xff" * 70, b"A" * m))
        pairs.append((_rand(rng, m, b"\xffA"), b"\xff" * 71))
        pairs.append((b"\xff" * 65, b"\xff" * m))
    pairs += [(b"\0" * 65, b"\0" * 130), (b"\0" * 130, b"\0A" * 33)]
    t = _rand(rng, 300)
    pairs += [(_mut_to(rng, t, 280).lower(), t), (bytes(c | 0x20 if rng.random() < 0.5 else c for c in t), t)]
    _check(pairs)


def _two_hundred():
    """200 pairs of 0..150 bases, related and unrelated; empty on one side or both at the ends of k_aln_trace's blocks of 64 threads"""
    rng = random.Random(105)
    pairs = []
    for k in range(200):
        t = _rand(rng, rng.randint(0, 150))
        pairs.append((_mut(rng, t, 0.2)[:150] if k % 2 else _rand(rng, rng.randint(0, 150)), t))
    for k, side in zip((0, 63, 64, 127, 128, 199), (0, 1, 2, 0, 1, 2)):
        q, t = pairs[k]
        pairs[k] = (b"" if side != 1 else q or b"A", b"" if side != 0 else t or b"A")
    return pairs


def test_more_pairs_than_one_trace_block(built):
    pairs = _two_hundred()
    assert len(pairs) == 200 and max(max(len(q), len(t)) for q, t in pairs) <= 150
    _check(pairs)


def _chunks(err):
    """VC_ALIGN_LOG lines -> [(first pair, pairs, matrix dwords)]"""
    out = []
    for line in err.splitlines():
        if line.startswith("vc_align: chunk "):
            d = dict(f.split("=", 1) for f in line.split()[2:])
            out.append((int(d["first"]), int(d["pairs"]), int(d["mat_dwords"])))
    return out


def _with_knobs(monkeypatch, capfd, call, **env):
    """call() under VC_ALIGN_LOG and the knobs env -> (its result, the chunks it logged)"""
    before = capfd.readouterr().out
    monkeypatch.setenv("VC_ALIGN_LOG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        res = call()
    finally:
        for k in _KNOBS:
            monkeypatch.delenv(k, raising=False)
    got = capfd.readouterr()
    print(before + got.out, end="")
    return res, _chunks(got.err)


def _batch_with_a_big_pair():
    rng = random.Random(106)
    small = _two_hundred()
    t = _rand(rng, 100)
    big = (_rand(rng, 700) + _mut_to(rng, t, 100) + _rand(rng, 700), t)             # 1500 x 100: 1.15 MB of stored matrix
    return small[:100] + [big] + small[100:], 100


def test_chunks_under_a_small_budget(built, monkeypatch, capfd):
    """VC_ALIGN_BUDGET_MB=1: the batch goes in many chunks (offset bases q_off + k0, skip + k0, results at edit_distance + k0) and the
    1.15 MB pair, over the budget by itself, runs alone; the answers are those of the one-chunk run and of the restatement"""
    from vechat_amd.align import align_pairs
    pairs, big = _batch_with_a_big_pair()
    plain = align_pairs(pairs)
    _compare(pairs, *plain)
    chunked, chunks = _with_knobs(monkeypatch, capfd, lambda: align_pairs(pairs), VC_ALIGN_BUDGET_MB=1)
    assert chunked == plain
    _compare(pairs, *chunked)
    assert len(chunks) > 1
    first = 0
    for k0, nj, dw in chunks:                                   # the chunks tile the batch in order ...
        assert k0 == first and nj >= 1
        assert dw * 4 <= 1 << 20 or nj == 1                     # ... each within the budget, or a single pair
        first += nj
    assert first == len(pairs)
    lone = [c for c in chunks if c[0] == big]
    assert lone == [(big, 1, 1500 * 192)]
    assert sum(1 for c in chunks if c[2] * 4 > 1 << 20) == 1


def test_a_pair_outside_the_envelope_is_reported_not_guessed(built, monkeypatch, capfd):
    """VC_ALIGN_MAX_MAT_MB=1: the pair whose matrix is larger comes back with distance -1 and no CIGAR, an empty job on the device;
    every other pair of the call is unchanged"""
    from vechat_amd.align import align_pairs
    pairs, big = _batch_with_a_big_pair()
    (cigars, dist), chunks = _with_knobs(monkeypatch, capfd, lambda: align_pairs(pairs), VC_ALIGN_MAX_MAT_MB=1)
    assert dist[big] == -1 and cigars[big] == ""
    _compare(pairs, cigars, dist, except_for=(big,))
    assert sum(c[1] for c in chunks) == len(pairs) and sum(c[2] for c in chunks) == sum(len(q) * 192 for q, t in pairs if t) - 1500 * 192
    _check(pairs)                                               # and without the knob it is aligned again


def test_align_missing_drops_an_overlap_outside_the_envelope(built, monkeypatch, capfd):
    """seqio.align_missing on the device: distance < 0 means drop (error 2.0, empty CIGAR), the other overlaps get their CIGARs --
    of the pieces the record names, reverse-complemented for strand '-'"""
    from vechat_amd import seqio
    rng = random.Random(107)
    tgt = _rand(rng, 2000)
    rc = lambda s: s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    r_fwd = _rand(rng, 20) + _mut_to(rng, tgt[100:400], 300) + _rand(rng, 10)
    r_rev = rc(_mut_to(rng, tgt[1200:1500], 310))
    r_big = _mut_to(rng, tgt[300:1800], 1500, 0.05)
    targets = [("t0", tgt, None)]
    reads = [("fwd", r_fwd, None), ("rev", r_rev, None), ("big", r_big, None)]
    mk = lambda name, strand, qb, qe, ql, tb, te: seqio.Overlap(q_name=name, t_name="t0", strand=strand, q_begin=qb, q_end=qe, q_length=ql,
                                                               t_begin=tb, t_end=te, cigar=None, length=max(qe - qb, te - tb),
                                                               error=1 - min(qe - qb, te - tb) / float(max(qe - qb, te - tb)))
    ovl = [mk("fwd", False, 20, 320, len(r_fwd), 100, 400), mk("big", False, 0, 1500, 1500, 300, 1800), mk("rev", True, 0, 310, 310, 1200, 1500)]
    assert 1500 * 192 * 4 > 1 << 20 > 310 * 192 * 4
    n_ok, _ = _with_knobs(monkeypatch, capfd, lambda: seqio.align_missing(targets, reads, ovl), VC_ALIGN_MAX_MAT_MB=1)
    assert n_ok == 2
    assert ovl[1].error == 2.0 and ovl[1].cigar == ""
    assert ovl[0].cigar == _ref(r_fwd[20:320], tgt[100:400])[0] and ovl[0].error < 0.3
    assert ovl[2].cigar == _ref(rc(r_rev), tgt[1200:1500])[0] and ovl[2].error < 0.3


# ---------------------------------------------------------------------------------------------------------------------------
# The C ABI itself
VC_OK, VC_ERR_ARG, VC_ERR_HIP = 0, -1, -2


class _Call:
    """one vc_align call through ctypes with every argument in the open"""

    def __init__(self, pairs, cap=None):
        from vechat_amd import capi
        from vechat_amd.align import VcAlignBatch
        self.lib = lib = capi.load_hip()
        lib.vc_align.argtypes = [C.c_int, C.POINTER(VcAlignBatch), C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        lib.vc_align.restype = C.c_int
        lib.vc_align_last_error.restype = C.c_char_p
        n = self.n = len(pairs)
        self.qo = np.zeros(n + 1, np.uint64); self.to = np.zeros(n + 1, np.uint64)
        self.qo[1:] = np.cumsum([len(q) for q, _ in pairs]); self.to[1:] = np.cumsum([len(t) for _, t in pairs])
        self.qb = np.frombuffer(b"".join(q for q, _ in pairs) + b"\0", np.uint8).copy()
        self.tb = np.frombuffer(b"".join(t for _, t in pairs) + b"\0", np.uint8).copy()
        p8, p64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        self.batch = VcAlignBatch(n, self.qo.ctypes.data_as(p64), self.qb.ctypes.data_as(p8), self.to.ctypes.data_as(p64), self.tb.ctypes.data_as(p8))
        self.cap = int(self.qo[-1] + self.to[-1]) * 6 + 16 * n + 64 if cap is None else cap
        self.buf = C.create_string_buffer(self.cap + 8)                                 # 8 guard bytes behind the capacity
        self.buf.raw = b"\xa5" * (self.cap + 8)
        self.off = np.full(n + 1, 0xDEAD, np.uint64)
        self.dist = np.full(n, -77, np.int32)

    def run(self, batch=True, off=True, dist=True):
        rc = self.lib.vc_align(0, C.byref(self.batch) if batch else None, self.buf, self.cap,
                               self.off.ctypes.data_as(C.POINTER(C.c_uint64)) if off else None,
                               self.dist.ctypes.data_as(C.POINTER(C.c_int32)) if dist else None)
        assert self.buf.raw[self.cap:] == b"\xa5" * 8                                   # nothing written behind the capacity
        return rc

    def answers(self):
        raw = self.buf.raw
        return [raw[int(self.off[k]):int(self.off[k + 1]) - 1].decode() for k in range(self.n)], [int(x) for x in self.dist]


def test_abi_empty_batch_and_null_arguments(built):
    pairs = [(q, t) for q, t, _, _ in KNOWN]
    c = _Call([])
    assert c.run() == VC_OK and int(c.off[0]) == 0
    c = _Call(pairs)
    assert c.run(batch=False) == VC_ERR_ARG
    assert c.run(off=False) == VC_ERR_ARG
    assert c.run(dist=False) == VC_ERR_ARG
    assert c.run() == VC_OK                                     # the refused calls left nothing behind that would break the next
    _compare(pairs, *c.answers())


def test_abi_cigar_buffer_one_byte_short(built):
    rng = random.Random(108)
    pairs = _two_hundred()[:70] + [(_rand(rng, 300), _rand(rng, 2100))]
    need = sum(len(_ref(q, t)[0]) + 1 for q, t in pairs)
    c = _Call(pairs, cap=need - 1)
    assert c.run() == VC_ERR_HIP
    assert b"cigar buffer too small" in c.lib.vc_align_last_error()
    c = _Call(pairs, cap=need)                                  # exactly enough
    assert c.run() == VC_OK
    assert int(c.off[-1]) == need
    _compare(pairs, *c.answers())


def test_release_and_regrowth_of_the_matrix_buffer(built, monkeypatch, capfd):
    """the cached matrix buffer: made, regrown for a larger call, reused by a smaller one, released, made again -- the answers never
    change.  (The VC_ALIGN_LOG lines give each call's matrix size: the order below is small, larger, small, release, largest, small.)"""
    from vechat_amd import align
    rng = random.Random(109)
    small = _two_hundred()[60:70]
    t1, t2 = _rand(rng, 2500), _rand(rng, 4200)
    larger = small[:3] + [(_mut_to(rng, t1, 700), t1)] + small[3:6]
    largest = [(_mut_to(rng, t2, 1300), t2)] + small
    align.release()                                             # whatever earlier tests left
    sizes = []
    for step in (small, larger, small, None, largest, small, None):
        if step is None:
            align.release()
            continue
        _, chunks = _with_knobs(monkeypatch, capfd, lambda: _check(step))
        assert len(chunks) == 1
        sizes.append(chunks[0][2])
    assert sizes[0] < sizes[1] < sizes[3] and sizes[0] == sizes[2] == sizes[4]
