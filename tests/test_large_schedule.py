"""GPU suite (-m gpu): the host schedule of the large-graph path (vc_large_run) -- table regrowth, groups of windows, forward
launches split by the matrix budget, the arena refusal, the buffer cache across calls -- and windows at the edge shapes of k_lg_fwd
and k_lg_back.  Small windows reach the rare paths through the path's development knobs (VC_LARGE_CAPS, VC_LARGE_ARENA_MB,
VC_LARGE_MAT_MB; header of vc_large.hip), and every test reads the VC_LARGE_LOG lines to prove that the path it aims at ran.
Bar: test_large_graphs._expect, i.e. the oracle's consensus bytes and status for every window."""
from collections import Counter

import numpy as np
import pytest

import oracle_api as oa
from test_large_graphs import _expect, _iupac
from vechat_amd import capi, large
from vechat_amd.engine import HipContext

pytestmark = pytest.mark.gpu

_ENV = dict(caps="VC_LARGE_CAPS", arena_mb="VC_LARGE_ARENA_MB", mat_mb="VC_LARGE_MAT_MB", log="VC_LARGE_LOG")
_FLAG = dict(n="nodes", e="edges", a="aligned", l="labels", s="stack", p="pairs")
# shifts that leave every table of _mix() below half of what some window needs, so that it regrows at least twice
_SHIFT = dict(n=5, e=5, a=7, l=3, s=10, p=6)


def _knobs(monkeypatch, **kw):
    for v in _ENV.values():
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(_ENV["log"], "1")
    for k, v in kw.items():
        monkeypatch.setenv(_ENV[k], str(v))


def _events(err):
    """VC_LARGE_LOG lines -> [(event, {key: value})]"""
    out = []
    for line in err.splitlines():
        if line.startswith("vc_large: "):
            kind, *rest = line[len("vc_large: "):].split()
            out.append((kind, dict(t.split("=", 1) for t in rest if "=" in t)))
    return out


def _run(monkeypatch, capfd, batch, params, **kw):
    """large_consensus under VC_LARGE_LOG=1 and the knobs kw (caps=, arena_mb=, mat_mb=) -> (cons, status, events)"""
    _knobs(monkeypatch, **kw)
    before = capfd.readouterr().out
    try:
        cons, status = large.large_consensus(batch, params)
    finally:
        for v in _ENV.values():
            monkeypatch.delenv(v, raising=False)
    got = capfd.readouterr()
    print(before + got.out, end="")             # what the test printed so far stays in its captured output
    return cons, status, _events(got.err)


def _regrows(ev):
    return [(int(d["window"]), set(d["flags"].split(","))) for k, d in ev if k == "regrow"]


def _groups(ev):
    """[(window ids, table bytes of each)] in launch order"""
    return [([int(x) for x in d["ids"].split(",")], [int(x) for x in d["need"].split(",")]) for k, d in ev if k == "group"]


def _summary(ev):
    c = Counter(k for k, _ in ev)
    flags = Counter(f for _, fl in _regrows(ev) for f in fl)
    return f"{dict(c)} flags={dict(flags)} groups={[len(ids) for ids, _ in _groups(ev)]}"


def _join(*batches):
    wins, fl = [], []
    for b in batches:
        for w in range(b.n_windows):
            wins.append(b.window(w))
            fl.append(int(b.win_fasta[w]))
    return capi.Batch.from_windows(wins, fl, presorted=True)


# ------------------------------------------------------------------ windows built here (seeded)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _rand(rng, n):
    return bytes(rng.choice(_ACGT, n))


def _noisy(rng, s, sub=0.0, indel=0.0):
    """s with substitutions (rate sub) and single-base insertions / deletions (rate indel, half each)"""
    out = []
    for c in s:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(int(rng.choice(_ACGT)))
        out.append(int(rng.choice(_ACGT[_ACGT != c])) if rng.random() < sub else c)
    return bytes(out) or s[:1]


def _window(rng, backbone, layers, fasta=False):
    """(seqs, quals, begins, ends) for Batch.from_windows; layers = [(sequence, begin, end)].  FASTA: no layer qualities and the
    dummy '!' backbone quality (polisher.cpp:181)."""
    L = len(backbone)
    q = lambda n: bytes(rng.integers(33 + 5, 33 + 41, n).astype(np.uint8))
    seqs = [backbone] + [s for s, _, _ in layers]
    quals = [b"!" * L if fasta else q(L)] + [None if fasta else q(len(s)) for s, _, _ in layers]
    return seqs, quals, [0] + [b for _, b, _ in layers], [0] + [e for _, _, e in layers]


def _batch(wins):
    return capi.Batch.from_windows([w for w, _ in wins], [int(f) for _, f in wins])


@pytest.fixture(scope="module")
def mix():
    """5 windows of 160-380 bp at 12-28x: partial-span layers, a FASTA-layer window, two haplotypes, and one IUPAC window"""
    return _join(capi.synth_batch(capi.synth_cfg(601, 250, 20, frac_partial=0.3), 0, 2),
                 capi.synth_batch(capi.synth_cfg(602, 380, 12, frac_partial=0.4, fastq=0), 0, 1),
                 capi.synth_batch(capi.synth_cfg(603, 160, 28, n_haplotypes=2, snp_rate=0.03, frac_partial=0.2), 0, 1),
                 _iupac(capi.synth_batch(capi.synth_cfg(604, 200, 16, frac_partial=0.3), 0, 1), b"ACGTURYSWKMBDHVN", 0.35, 7))


# ------------------------------------------------------------------ 1. every table regrows
@pytest.mark.parametrize("mode,tables", [(0, t) for t in "neasp"] + [(1, t) for t in "nealsp"] + [(0, "neasp"), (1, "nealsp")])
def test_each_table_regrows_and_the_bytes_stay(built, monkeypatch, capfd, mix, mode, tables):
    caps = ",".join(f"{t}:{_SHIFT[t]}" for t in tables)
    p = capi.default_params(mode=mode)
    cons, status, ev = _run(monkeypatch, capfd, mix, p, caps=caps)
    print(f"[regrow {caps} mode {mode}] {_summary(ev)}")
    rg = _regrows(ev)
    seen = set().union(*(f for _, f in rg)) if rg else set()
    for t in tables:
        assert _FLAG[t] in seen, (caps, seen)
    assert max(Counter(w for w, _ in rg).values()) >= 2, rg
    _expect(mix, p, cons, status, f"caps {caps} mode{mode}")


# ------------------------------------------------------------------ 2. one window regrows while the others of its group finish
@pytest.mark.parametrize("noisy_at", [3, 0])
def test_a_regrown_window_runs_again_alone(built, monkeypatch, capfd, noisy_at):
    rng = np.random.default_rng(202)
    wins = []
    for _ in range(3):                          # near-copies of the backbone: the graph stays near L nodes
        bb = _rand(rng, 200)
        wins.append((_window(rng, bb, [(_noisy(rng, bb, sub=0.01), 0, 199) for _ in range(10)]), 0))
    noisy = capi.synth_batch(capi.synth_cfg(205, 200, 10), 0, 1)
    wins.insert(noisy_at, (noisy.window(0), int(noisy.win_fasta[0])))
    batch = _batch(wins)
    p = capi.default_params()
    # the node table's initial size is (bases of the window + 1) >> shift: pick the shift that holds the near-copies' graphs but
    # not the noisy window's (the oracle's build graphs are the largest the window makes)
    sums = [int(batch.seq_off[batch.win_seq_off[w + 1]] - batch.seq_off[batch.win_seq_off[w]]) for w in range(4)]
    need = [oa.oracle_run(batch, p, w, w + 1)[2].max_nodes for w in range(4)]
    fits = lambda s, w: (sums[w] + 1) >> s >= need[w]
    shift = next(s for s in range(1, 12) if not fits(s, noisy_at) and all(fits(s, w) for w in range(4) if w != noisy_at))
    cons, status, ev = _run(monkeypatch, capfd, batch, p, caps=f"n:{shift}")
    print(f"[lock-step regrow, noisy window {noisy_at}, n:{shift}] {_summary(ev)}")
    groups, rg = _groups(ev), _regrows(ev)
    assert sorted(groups[0][0]) == [0, 1, 2, 3]
    assert rg and {w for w, _ in rg} == {noisy_at}
    assert len(groups) == 1 + len(rg) and all(ids == [noisy_at] for ids, _ in groups[1:])
    _expect(batch, p, cons, status, f"lock-step regrow at {noisy_at}")


# ------------------------------------------------------------------ 3. groups under a small arena budget
def _ragged12():
    """the shapes of test_ragged_and_wide_alphabet_windows_through_the_large_path, three windows each, large ones first"""
    shapes = [(300, 30, 0.2), (80, 1, 0), (64, 2, 0), (150, 3, 0.5)]
    parts = [capi.synth_batch(capi.synth_cfg(70 + i, L, D, frac_partial=fp), 0, 3) for i, (L, D, fp) in enumerate(shapes)]
    return _join(*parts)


def test_groups_under_a_small_arena_budget(built, monkeypatch, capfd):
    batch = _ragged12()
    big, small = [0, 1, 2], list(range(3, 12))
    for mode in (0, 1):
        p = capi.default_params(mode=mode)
        c0, s0, ev0 = _run(monkeypatch, capfd, batch, p)
        assert len(_groups(ev0)) == 1 and not _regrows(ev0)
        _expect(batch, p, c0, s0, f"ragged12 default mode{mode}")
        # the node table at a quarter: the windows of 1 and 2 layers regrow (the backbone alone fills it)
        c1, s1, ev1 = _run(monkeypatch, capfd, batch, p, caps="n:2")
        ids, need = _groups(ev1)[0]
        nb = dict(zip(ids, need))
        assert sorted(ids) == list(range(12)) and _regrows(ev1)
        # the first large window and every small one fit; a second large one does not; a large one beside the regrown small
        # ones does
        ssum = sum(nb[w] for w in small)
        budget = max(nb[w] for w in big) + 2 * ssum
        assert min(nb[w] for w in big) > 2 * ssum, nb
        c2, s2, ev2 = _run(monkeypatch, capfd, batch, p, caps="n:2", arena_mb=f"{budget / 2**20:.6f}")
        print(f"[groups mode {mode}, arena {budget} B] {_summary(ev2)}")
        groups = [ids for ids, _ in _groups(ev2)]
        assert len(groups) >= 3 and max(len(g) for g in groups) > 1, groups
        ran, shared = set(), False
        for g in groups:
            shared |= any(w in ran for w in g) and any(w not in ran for w in g)
            ran |= set(g)
        assert shared, groups                   # a regrown window shared a group with windows on their first attempt
        assert c2 == c0 and (s2 == s0).all() and c1 == c0 and (s1 == s0).all()
        _expect(batch, p, c2, s2, f"ragged12 groups mode{mode}")


# ------------------------------------------------------------------ 4. steps split into several forward launches
@pytest.mark.parametrize("mode", [0, 1])
def test_steps_split_under_a_small_matrix_budget(built, monkeypatch, capfd, mode):
    # the 300 bp window's matrices (>= 301 x 301 int32 cells) are above 0.25 MiB from its first alignment on; the 150 bp ones
    # are below
    batch = _join(capi.synth_batch(capi.synth_cfg(401, 150, 10, frac_partial=0.3), 0, 2),
                  capi.synth_batch(capi.synth_cfg(402, 300, 16), 0, 1),
                  capi.synth_batch(capi.synth_cfg(403, 150, 10, fastq=0), 0, 2))
    p = capi.default_params(mode=mode)
    cons, status, ev = _run(monkeypatch, capfd, batch, p, mat_mb=0.25)
    print(f"[split launches mode {mode}] {_summary(ev)}")
    steps = [d for k, d in ev if k == "step"]
    assert steps and max(int(d["launches"]) for d in steps) >= 3
    assert any(int(d["over"]) >= 1 for d in steps)
    _expect(batch, p, cons, status, f"split launches mode{mode}")


# ------------------------------------------------------------------ 5. a window above twice the arena budget is refused
def _long_layer_batch():
    """the batch of test_large_graphs.test_the_long_layer_window_through_the_large_path: window 2 holds a 40 kb layer (about
    11 MiB of tables); the others about 0.7 MiB each"""
    good = capi.synth_batch(capi.synth_cfg(83, 300, 8), 0, 4)
    wins = [good.window(w) for w in range(4)]
    seqs, quals, b, e = wins[2]
    huge = (seqs[1] * 200)[:40000]
    wins[2] = (seqs[:2] + [huge] + seqs[2:], quals[:2] + [b"5" * len(huge)] + quals[2:], b[:2] + [0] + b[2:],
               e[:2] + [len(seqs[0]) - 1] + e[2:])
    return capi.Batch.from_windows(wins, [int(good.win_fasta[w]) for w in range(4)])


def test_a_window_above_the_arena_budget_is_refused(built, monkeypatch, capfd):
    batch = _long_layer_batch()
    p = capi.default_params()
    cons, status, ev = _run(monkeypatch, capfd, batch, p, arena_mb=1)
    print(f"[arena refusal, large_consensus] {_summary(ev)}")
    assert [int(d["window"]) for k, d in ev if k == "refuse"] == [2]
    assert int(status[2]) == capi.VC_WIN_OVERFLOW and cons[2] == b""
    keep = [0, 1, 3]
    _expect(batch.select(keep), p, [cons[w] for w in keep], status[keep], "beside the refused window")


def test_the_context_leaves_a_refused_window_overflowed(built, monkeypatch, capfd):
    batch = _long_layer_batch()
    _knobs(monkeypatch, arena_mb=1)
    ctx = HipContext(device=0)
    try:
        cons, status = ctx.consensus(batch)
    finally:
        ctx.close()
        monkeypatch.delenv(_ENV["arena_mb"])
    ev = _events(capfd.readouterr().err)
    print(f"[arena refusal, HipContext] {_summary(ev)}")
    assert [int(d["window"]) for k, d in ev if k == "refuse"] == [0]      # the only window of the large-path call
    assert int(status[2]) == capi.VC_WIN_OVERFLOW and ctx.large_windows == 0
    keep = [0, 1, 3]
    _expect(batch.select(keep), capi.default_params(), [cons[w] for w in keep], status[keep], "context beside the refused window")


# ------------------------------------------------------------------ 6. the grow-only buffer cache across calls
def test_the_buffer_cache_across_calls(built, monkeypatch, capfd):
    small = capi.synth_batch(capi.synth_cfg(901, 150, 8, frac_partial=0.3), 0, 2)
    big = capi.synth_batch(capi.synth_cfg(902, 900, 24, frac_partial=0.2), 0, 2)
    p = capi.default_params()
    large.release()
    used = []
    for label, batch in (("small", small), ("large", big), ("small again", small)):
        cons, status, ev = _run(monkeypatch, capfd, batch, p)
        _expect(batch, p, cons, status, label)
        used.append(sum(sum(n) for _, n in _groups(ev)))
    print(f"[buffer cache] table bytes per call: {used}")
    assert used[0] < used[1] and used[2] == used[0]
    large.release()
    cons, status, _ = _run(monkeypatch, capfd, big, p)
    _expect(big, p, cons, status, "after release")


# ------------------------------------------------------------------ 7. edge shapes, through both device paths
_LENS = (1, 2, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)


def _edge_windows():
    """Seeded windows at k_lg_fwd's lane (8 columns) and chunk (512 columns) boundaries, and repeats full of co-optimal paths."""
    rng = np.random.default_rng(77)
    wins = []
    for k, n in enumerate(_LENS):
        fasta = k % 2 == 1
        L = max(n, 24)
        bb = _rand(rng, L)
        lay = []
        for d in range(6):                      # layers of exactly n bases: full-span, and partial ones at both ends
            b0 = int(rng.integers(0, L - n + 1))
            s = _noisy(rng, bb[b0:b0 + n], sub=0.08)
            pos = [(0, L - 1), (0, L - 1), (0, max(1, L // 2)), (min(L // 2, L - 2), L - 1)][d % 4]
            lay.append((s, *pos))
        if n >= 63:                             # reads with indels around n, and one a third long
            lay += [(_noisy(rng, bb, sub=0.03, indel=0.04), 0, L - 1) for _ in range(3)]
            lay.append((_noisy(rng, bb[n // 3:2 * n // 3], sub=0.05), n // 3, 2 * n // 3))
        b1 = int(rng.integers(0, L - 1))
        lay.append((bb[b1:b1 + 1], b1, b1 + 1))                               # a one-base layer
        wins.append((_window(rng, bb, lay, fasta), fasta))
    # homopolymers: one letter, and runs whose lengths the reads shift by one
    hp = b"A" * 150
    wins.append((_window(rng, hp, [(b"A" * (150 + d), 0, 149) for d in (-3, -1, 0, 1, 2, 4)] + [(b"A" * 40, 20, 60), (b"A", 0, 1)]), 0))
    runs = [(int(rng.choice(_ACGT)), int(rng.integers(2, 9))) for _ in range(45)]
    mk = lambda rr: bytes(c for c, m in rr for _ in range(m))
    hb = mk(runs)
    reads = [(mk([(c, max(1, m + int(rng.integers(-1, 2)))) for c, m in runs]), 0, len(hb) - 1) for _ in range(9)]
    wins.append((_window(rng, hb, reads + [(mk(runs[10:20]), len(mk(runs[:10])), len(mk(runs[:20])))], fasta=True), 1))
    # dinucleotide repeats: reads that start a base later, or gain or lose a unit
    dn = b"AC" * 110
    reads = [(b"CA" * 110, 0, 219), (b"C" + b"AC" * 109, 0, 219), (b"AC" * 111, 0, 219), (b"AC" * 108, 0, 219),
             (b"AC" * 50 + b"A" + b"AC" * 60, 0, 219), (b"AC" * 110, 0, 219), (b"CACA" * 20, 100, 219), (b"AC" * 30, 0, 59)]
    wins.append((_window(rng, dn, reads), 0))
    at = b"AT" * 60 + _rand(rng, 60) + b"GT" * 40
    reads = [(_noisy(rng, at, indel=0.05), 0, len(at) - 1) for _ in range(8)] + [(b"TA" * 30, 0, 60)]
    wins.append((_window(rng, at, reads), 0))
    return _batch(wins)


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_shape_windows_through_both_device_paths(built, monkeypatch, capfd, mode):
    batch = _edge_windows()
    p = capi.default_params(mode=mode)
    cons, status, ev = _run(monkeypatch, capfd, batch, p)
    assert len(_groups(ev)) == 1 and not _regrows(ev)
    _expect(batch, p, cons, status, f"edge shapes, large path, mode{mode}")
    ctx = HipContext(device=0, mode=mode)
    try:
        fc, fs = ctx.consensus(batch)
    finally:
        ctx.close()
    _expect(batch, p, fc, fs, f"edge shapes, fast path, mode{mode}")
    print(f"[edge shapes mode {mode}] {batch.n_windows} windows, large path and fast path equal the oracle")
    if oa.have_ref():                           # the independent judge of the tie rules the oracle shares with the kernels
        for w in range(0, batch.n_windows, 2):
            got, pol = oa.ref_window(batch, w, p)
            assert cons[w] == got and (int(status[w]) == capi.VC_WIN_OK) == bool(pol), (mode, w)


# ------------------------------------------------------------------ 8. the int32 score floor
def test_the_score_floor(built, monkeypatch, capfd):
    """AlignmentEngine::WorstCaseAlignmentScore (vc_large.hip worst_case, vc_oracle.c:257) against KNEG: the most negative gap
    score the oracle takes for this window, by bisection; one below it the oracle refuses (vco_run fails) and the large path
    returns VC_WIN_INVALID."""
    batch = capi.synth_batch(capi.synth_cfg(808, 150, 10, frac_partial=0.3), 0, 1)
    params = lambda g: capi.default_params(gap=g, sw_gap=g)

    def takes(g):
        try:
            oa.oracle_run(batch, params(g))
            return True
        except RuntimeError:
            return False
    ok, bad = -4, -(1 << 30)
    assert takes(ok) and not takes(bad)
    while ok - bad > 1:
        mid = (ok + bad) // 2
        ok, bad = (mid, bad) if takes(mid) else (ok, mid)
    cons, status, _ = _run(monkeypatch, capfd, batch, params(ok))
    _expect(batch, params(ok), cons, status, f"gap {ok}")
    cons, status, _ = _run(monkeypatch, capfd, batch, params(bad))
    assert int(status[0]) == capi.VC_WIN_INVALID and cons[0] == b""
    print(f"[score floor] gap {ok}: the oracle's bytes; gap {bad}: VC_WIN_INVALID")
