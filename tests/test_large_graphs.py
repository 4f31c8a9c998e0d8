"""GPU suite (-m gpu): the large-graph path (vc_large_run) -- windows the fast path's 16-bit tables cannot hold -- against the
oracle, the golden fixtures and, where it was built, the reference itself.  Bar: bit-exact consensus bytes and status."""
import gzip
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
import oracle_api as oa
from vechat_amd import capi, large
from vechat_amd.engine import MAX_EDGES, HipContext

pytestmark = pytest.mark.gpu


def _oracle(batch, params, threads=16):
    """oracle_run over the windows of batch, in slices on several threads (the calls release the GIL)."""
    n = batch.n_windows
    cuts = sorted({round(k * n / threads) for k in range(threads + 1)})
    with ThreadPoolExecutor(len(cuts) - 1) as ex:
        parts = list(ex.map(lambda c: oa.oracle_run(batch, params, c[0], c[1]), zip(cuts[:-1], cuts[1:])))
    cons = [x for p in parts for x in p[0]]
    pol = np.concatenate([p[1] for p in parts])
    return cons, pol, [p[2] for p in parts]


def _expect(batch, params, cons, status, label):
    ref, pol, _ = _oracle(batch, params)
    for w in range(batch.n_windows):
        assert int(status[w]) == (capi.VC_WIN_OK if pol[w] else capi.VC_WIN_UNPOLISHED), (label, w, int(status[w]))
        assert cons[w] == ref[w], (label, w, len(cons[w]), len(ref[w]))


# ------------------------------------------------------------------ 1. ordinary windows, forced through the large path
@pytest.mark.parametrize("mode,key", [(0, "hap"), (1, "linear")])
def test_golden_windows_through_the_large_path(built, mode, key):
    gold = fixtures.load_windows()
    batch = fixtures.fixture_batch(gold["windows"])
    p = capi.default_params(mode=mode)
    cons, status = large.large_consensus(batch, p)
    for w, win in enumerate(gold["windows"]):
        exp = win["expected"][key]
        assert cons[w].decode() == exp["consensus"], win["name"]
        assert (int(status[w]) == capi.VC_WIN_OK) == exp["polished"], win["name"]
    _expect(batch, p, cons, status, f"golden mode{mode}")


def _iupac(batch, alphabet, rate, seed):
    from test_gpu import _recode
    return _recode(batch, alphabet, rate, seed)


@pytest.mark.parametrize("cfg,n,kw", [
    (capi.synth_cfg(3, 200, 12, frac_partial=0.3), 8, {}),
    (capi.synth_cfg(13, 500, 40, n_haplotypes=2, snp_rate=0.02, frac_partial=0.2), 4, {}),
    (capi.synth_cfg(2, 60, 5, fastq=0, backbone_fastq=0), 8, {}),                              # FASTA backbones and reads
    (capi.synth_cfg(17, 250, 20, fastq=0, backbone_fastq=1, frac_partial=0.25), 6, {}),
    (capi.synth_cfg(77, 250, 12, frac_partial=0.5, fastq=0, backbone_fastq=0), 8, dict(mode=1)),
    (capi.synth_cfg(1002, 500, 64), 3, dict(mode=1, trim=1, window_type=1)),                   # racon-linear, TGS trim
    (capi.synth_cfg(1003, 300, 20, frac_partial=0.3), 4, dict(mode=1, trim=1, window_type=0)),
    (capi.synth_cfg(41, 180, 14, n_haplotypes=2, snp_rate=0.03), 4, dict(num_prune=4, min_confidence=0.22, min_support=0.19)),
    (capi.synth_cfg(41, 180, 14, n_haplotypes=2, snp_rate=0.03), 4, dict(num_prune=1)),
    (capi.synth_cfg(3003, 300, 16, frac_partial=0.3), 4, dict(match=2, mismatch=-3, gap=-12, sw_match=4, sw_mismatch=1, sw_gap=-2)),
])
def test_seeded_windows_through_the_large_path(built, cfg, n, kw):
    batch = capi.synth_batch(cfg, 0, n)
    p = capi.default_params(**kw)
    cons, status = large.large_consensus(batch, p)
    _expect(batch, p, cons, status, str(kw))


def test_ragged_and_wide_alphabet_windows_through_the_large_path(built):
    parts = [capi.synth_batch(capi.synth_cfg(50 + i, L, D, frac_partial=fp), 0, 2)
             for i, (L, D, fp) in enumerate([(80, 1, 0), (300, 30, 0.2), (64, 2, 0), (150, 3, 0.5)])]
    wins, fl = [], []
    for b in parts:
        for w in range(b.n_windows):
            wins.append(b.window(w)); fl.append(int(b.win_fasta[w]))
    ragged = capi.Batch.from_windows(wins, fl, presorted=True)
    base = capi.synth_batch(capi.synth_cfg(301, 160, 40, frac_partial=0.2), 0, 4)
    iupac = _iupac(base, b"ACGTURYSWKMBDHVN", 0.35, 5)
    for label, batch in (("ragged", ragged), ("iupac", iupac)):
        for mode in (0, 1):
            p = capi.default_params(mode=mode)
            cons, status = large.large_consensus(batch, p)
            _expect(batch, p, cons, status, f"{label} mode{mode}")


# ------------------------------------------------------------------ 2. beyond the edge ceiling, through the context
@pytest.fixture(scope="module")
def big():
    """One synth_cfg(7, 5000, 64) window (PacBio profile, 15 % error: ~17.6 k nodes, ~38.8 k edges) and its oracle result."""
    batch = capi.synth_batch(capi.synth_cfg(7, 5000, 64), 0, 1)
    p = capi.default_params()
    ref, pol, st = oa.oracle_run(batch, p)
    assert st.max_edges > MAX_EDGES, st.max_edges
    return batch, ref, pol


def test_a_window_beyond_the_edge_ceiling_is_computed(built, big):
    batch, ref, pol = big
    ctx = HipContext(device=0)
    t0 = time.time()
    cons, status = ctx.consensus(batch)
    dt = time.time() - t0
    assert int(status[0]) == capi.VC_WIN_OK and pol[0] == 1
    assert cons[0] == ref[0], (len(cons[0]), len(ref[0]))
    assert ctx.large_windows == 1
    ctx.close()
    print(f"[large path] 5000 x 64 window, mode 0, through HipContext.consensus: {dt:.1f} s")


def test_the_reference_agrees_on_the_window_beyond_the_edge_ceiling(built, big):
    if not oa.have_ref():
        pytest.skip("oracle/_ref not built (no reference tree at build time)")
    batch, ref, _ = big
    got, pol = oa.ref_window(batch, 0, capi.default_params())[:2]
    assert got == ref[0] and pol


# ------------------------------------------------------------------ 3. beyond 16-bit ids
@pytest.mark.parametrize("mode", [0, 1])
def test_a_window_beyond_16_bit_ids(built, mode):
    batch = capi.synth_batch(capi.synth_cfg(7, 30000, 5), 0, 1)
    p = capi.default_params(mode=mode)
    ref, pol, st = oa.oracle_run(batch, p)
    if mode == 0:           # (the oracle records graph sizes in the haplotype overload; the racon-linear one builds the same graph)
        assert max(st.max_nodes, st.max_edges) > 65535, (st.max_nodes, st.max_edges)
    t0 = time.time()
    cons, status = large.large_consensus(batch, p)
    dt = time.time() - t0
    large.release()
    assert int(status[0]) == capi.VC_WIN_OK and pol[0] == 1
    assert cons[0] == ref[0], (len(cons[0]), len(ref[0]))
    print(f"[large path] 30000 x 5 window, mode {mode}, vc_large_run: {dt:.1f} s")


# ------------------------------------------------------------------ 4. a mixed batch, and the command line
def test_mixed_batch_sends_only_the_big_window_down_the_large_path(built, big):
    bigb, bigref, _ = big
    small = capi.synth_batch(capi.synth_cfg(1002, 500, 64), 0, 200)
    wins = [small.window(w) for w in range(small.n_windows)]
    fl = [int(x) for x in small.win_fasta]
    wins.insert(117, bigb.window(0)); fl.insert(117, int(bigb.win_fasta[0]))
    batch = capi.Batch.from_windows(wins, fl, presorted=True)
    ctx = HipContext(device=0)
    cons, status = ctx.consensus_batched(batch, batch_windows=64, first=32)
    assert ctx.large_windows == 1
    ctx.close()
    assert int(status[117]) == capi.VC_WIN_OK and cons[117] == bigref[0]
    rest = [w for w in range(batch.n_windows) if w != 117]
    sub = batch.select(rest)
    _expect(sub, capi.default_params(), [cons[w] for w in rest], status[rest], "config C beside the big window")


def _mutate(rng, target, err=0.15, ins=0.40, dele=0.30):
    """a read of the whole target with PacBio-like errors -> (read, CIGAR against the target)"""
    acgt = list(b"ACGT")
    ops, out = [], []
    i = 0
    while i < len(target):
        r = rng.random()
        if r < err * ins:
            out.append(acgt[int(rng.integers(4))]); ops.append("I")
            continue
        if r < err * (ins + dele):
            ops.append("D"); i += 1
            continue
        c = target[i]
        if r < err:
            c = [x for x in acgt if x != c][int(rng.integers(3))]
        out.append(c); ops.append("M"); i += 1
    cig, k = [], 0
    while k < len(ops):
        t = k
        while t < len(ops) and ops[t] == ops[k]:
            t += 1
        cig.append(f"{t - k}{ops[k]}")
        k = t
    if ops[0] != "M" or ops[-1] != "M":
        return _mutate(rng, target, err, ins, dele)
    return bytes(out), "".join(cig)


def test_command_line_polishes_a_5kb_window(built, tmp_path, capsys):
    """-w 5000 -p on one 5 kb target with 64 reads: the window is beyond the fast path's edge ceiling; the command computes it
    and exits 0 (it used to exit 3), and the text equals the reference polish loop's CPU output where that was built."""
    from vechat_amd import polish, seqio
    from vechat_amd.windows import WindowBuilder
    rng = np.random.default_rng(11)
    target = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000))
    tp, rp, op = tmp_path / "target.fasta", tmp_path / "reads.fastq.gz", tmp_path / "ovl.sam"
    tp.write_text(">tig1\n" + target.decode() + "\n")
    reads = [_mutate(rng, target) for _ in range(64)]
    with gzip.open(rp, "wt") as f:
        for k, (r, _) in enumerate(reads):
            q = "".join(chr(33 + int(x)) for x in rng.integers(12, 40, len(r)))
            f.write(f"@read{k}\n{r.decode()}\n+\n{q}\n")
    with open(op, "w") as f:
        f.write("@HD\tVN:1.6\n")
        for k, (_, cig) in enumerate(reads):
            f.write(f"read{k}\t0\ttig1\t1\t60\t{cig}\t*\t0\t0\t*\t*\n")
    argv = [str(rp), str(op), str(tp), "-w", "5000", "-p", "-d", "0.2", "-s", "0.2"]
    assert polish.main(argv) == 0
    out, err = capsys.readouterr()
    assert out.startswith(">tig1") and "(1 on the large-graph path)" in err, err
    if oa.have_adapter():
        targets, rds, ovl = seqio.read_sequences(tp), seqio.read_sequences(rp), seqio.read_overlaps(op)
        wb = WindowBuilder(5000, 10.0)
        kept, _ = seqio.load_polisher_input(wb, targets, rds, ovl)
        batch, ids = wb.build()
        wb.close()
        cpu, ncpu = oa.adapter_polish(batch, ids, ["tig1"], [kept], capi.default_params(mode=0), cpu_only=True)
        assert ncpu == batch.n_windows and cpu == out


# ------------------------------------------------------------------ 5. a layer too long for the fast path's LDS notes
def test_the_long_layer_window_through_the_large_path(built):
    """The window of test_a_layer_too_long_for_the_device_takes_only_its_window_out (a 40 kb layer: VC_WIN_OVERFLOW at submit)."""
    good = capi.synth_batch(capi.synth_cfg(83, 300, 8), 0, 4)
    wins = [good.window(w) for w in range(4)]
    seqs, quals, b, e = wins[2]
    huge = (seqs[1] * 200)[:40000]
    wins[2] = (seqs[:2] + [huge] + seqs[2:], quals[:2] + [b"5" * len(huge)] + quals[2:], b[:2] + [0] + b[2:], e[:2] + [len(seqs[0]) - 1] + e[2:])
    batch = capi.Batch.from_windows(wins, [int(good.win_fasta[w]) for w in range(4)])
    for mode in (0, 1):
        p = capi.default_params(mode=mode)
        cons, status = large.large_consensus(batch.select([2]), p)
        _expect(batch.select([2]), p, cons, status, f"40 kb layer mode{mode}")
    ctx = HipContext(device=0)
    cons, status = ctx.consensus(batch)
    assert ctx.large_windows == 1
    ctx.close()
    _expect(batch, capi.default_params(), cons, status, "40 kb layer through the context")
