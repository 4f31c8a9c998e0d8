"""GPU suite (-m gpu): haplotype-aware correction of every member of a POA group (vc_poa_run_correct, poa.poa_correct, the command
line's --correct) -- every entry of tests/golden/poa_correct.json.gz byte for byte, freshly seeded groups against the CPU
restatement tests/poa_correct_ref.py, the consensus against poa_consensus's, the lane, chunk and tile boundaries, the host schedule
under the development knobs, statuses, the calls without correction, the cross-check through the haplotype window overload, and
the command line.  Each test prints its time."""
import os
import random
import re
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import pytest

import poa_correct_ref as PC
from poa_common import MODELS, _done, _workers
from test_poa_correct import entries
from vechat_amd import capi, large, poa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = capi.VC_WIN_OK
DEFAULTS = (0.22, 0.19, 3)


def _correct(groups, t, scores, prune=DEFAULTS):
    """-> (list of poa.Corrected, group statuses)"""
    return poa.run_batch_correct(poa.group_batch(groups), capi.VcPoaGapParams(0, t, *scores), capi.VcPoaPruneParams(*prune))


def _flat(res):
    return [(c.consensus, c.reads, c.scores.tolist(), c.status.tolist()) for c in res]


def _log(err):
    m = re.findall(r"vc_large: correct jobs=(\d+) launches=(\d+) cells=(\d+) bytes=(\d+)", err)
    assert len(m) == 1, err
    return tuple(map(int, m[0]))


def _knobs(monkeypatch, capfd, env, f):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        capfd.readouterr()
        out = f()
        err = capfd.readouterr().err
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return out, err


def _noisy(rng, s, rate=0.06):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append(rng.choice(b"ACGT") if x < 2 * rate / 3 else ch)
        if 2 * rate / 3 <= x < rate:
            out.append(rng.choice(b"ACGT"))
    return bytes(out) or s[:1]


def _qual(rng, s):
    return bytes(rng.randint(35, 73) for _ in s)


def _fresh(seed, n, lo=60, hi=300, kmin=3, kmax=17, quality="mixed"):
    """n groups of kmin..kmax members of lo..hi bases: two haplotypes a few SNVs apart, 6 % noise; members with and without quality"""
    rng = random.Random(seed)
    groups = []
    for w in range(n):
        h0 = bytearray(rng.choice(b"ACGT") for _ in range(rng.randrange(lo, hi + 1)))
        h1 = bytearray(h0)
        for p in rng.sample(range(len(h0)), min(4, len(h0))):
            h1[p] = rng.choice(b"ACGT")
        g = []
        for i in range(rng.randrange(kmin, kmax + 1)):
            s = _noisy(rng, bytes(h1 if i % 2 else h0))
            q = quality == "all" or (quality == "mixed" and (w + i) % 3 == 0)
            g.append((s, _qual(rng, s) if q else None))
        groups.append(g)
    return groups


def _ref_job(a):
    g, t, scores, prune = a
    r = PC.correct_group(g, t, *scores, *prune)
    return r["consensus"], r["reads"], r["scores"], r["final_nodes"], r["pairs"]


def _refs(groups, t, scores, prune=DEFAULTS):
    with ProcessPoolExecutor(_workers()) as ex:
        return list(ex.map(_ref_job, [(g, t, scores, prune) for g in groups], chunksize=2))


def _same(res, refs, what):
    for w, (c, r) in enumerate(zip(res, refs)):
        assert c.consensus == r[0], (what, w, "consensus")
        assert c.status.tolist() == [OK] * len(c.reads), (what, w)
        assert c.reads == r[1], (what, w, "reads")
        assert c.scores.tolist() == r[2], (what, w, "scores")


# ------------------------------------------------------------------ 1. every fixture entry
@pytest.mark.parametrize("part", range(4))
def test_every_fixture_entry(built, part):
    """the entries by call (algorithm, scores, thresholds and rounds), a call each; the calls dealt over four cases"""
    t0 = time.time()
    calls = {}
    for label, mem, e in entries():
        calls.setdefault((e["type"], tuple(e["scores"]), (e["min_confidence"], e["min_support"], e["num_prune"])), []).append((label, mem, e))
    assert len(calls) >= 8
    calls = dict(sorted(calls.items())[part::4])
    n = 0
    for (t, scores, prune), es in calls.items():
        res, status = _correct([mem for _, mem, _ in es], t, scores, prune)
        assert status.tolist() == [OK] * len(es)
        for (label, mem, e), c in zip(es, res):
            assert c.status.tolist() == [OK] * len(mem), label
            assert PC.same(dict(consensus=c.consensus, reads=c.reads, scores=c.scores), e["expected"]) == "", label
            n += len(mem)
    print(f"[fixture, part {part}] {n} members in {len(calls)} calls: consensus, corrections and scores equal to the reference's, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 2. fresh groups against the restatement, 3. the consensus
@pytest.mark.parametrize("model,t", [("linear", 1), ("affine", 0), ("convex", 2)])
def test_fresh_groups_against_the_restatement(built, model, t):
    groups = _fresh(9100 + t, 100)
    scores = MODELS[model]
    t0 = time.time()
    res, status = _correct(groups, t, scores)
    t1 = time.time()
    assert status.tolist() == [OK] * len(groups)
    _same(res, _refs(groups, t, scores), model)
    changed = sum(r != s for c, g in zip(res, groups) for r, (s, _) in zip(c.reads, g))
    split = sum(len({r for r in c.reads if len(r) > 40}) > 1 for c in res)
    assert changed > 100 and split > 10
    print(f"[fresh groups, {model} gaps, algorithm {t}] {sum(len(g) for g in groups)} members of {len(groups)} groups: {changed} changed by "
          f"their correction, {split} groups keep more than one sequence; equal to the restatement; device {t1 - t0:.1f} s, "
          f"restatement {time.time() - t1:.1f} s")


@pytest.mark.parametrize("model", list(MODELS))
def test_the_consensus_is_poa_consensus_s(built, model):
    groups = _fresh(9200, 60, hi=150, kmax=9) + [[], [(b"", None)], [(b"ACGT", None)]]
    t0 = time.time()
    for t in (0, 1, 2):
        p = capi.VcPoaGapParams(0, t, *MODELS[model])
        cons, status = poa.run_batch(poa.group_batch(groups), p)
        for k in (1, 3):
            res, st = _correct(groups, t, MODELS[model], (0.22, 0.19, k))
            assert st.tolist() == status.tolist() == [OK] * len(groups)
            assert [c.consensus for c in res] == cons, (t, k)
    print(f"[consensus, {model} gaps] {len(groups)} groups, three algorithms, 1 and 3 rounds: the consensus of vc_poa_run_gaps, "
          f"{time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 4. boundaries
@pytest.mark.parametrize("model", list(MODELS))
def test_member_lengths_at_the_lane_and_chunk_boundaries(built, model):
    rng = random.Random(9300)
    groups = []
    for n in (63, 64, 65, 511, 512, 513):
        truth = bytes(rng.choice(b"ACGT") for _ in range(n + 40))
        groups.append([(_noisy(rng, truth, 0.04)[:n].ljust(n, b"A"), None) for _ in range(4)])
        assert {len(s) for s, _ in groups[-1]} == {n}
    t0 = time.time()
    for t in (0, 1):
        res, status = _correct(groups, t, MODELS[model])
        assert status.tolist() == [OK] * len(groups)
        _same(res, _refs(groups, t, MODELS[model]), (model, t))
    print(f"[member lengths, {model} gaps] 63 / 64 / 65 (lanes x 8 columns) and 511 / 512 / 513 (the 512-column chunk): equal to the "
          f"restatement, {time.time() - t0:.1f} s")


def _tile_groups():
    """per size n: six copies of a sequence and a probe of n bases, the sequence with runs of six N that the others lack"""
    rng = random.Random(9400)
    groups = []
    for n in (63, 64, 65, 127, 128, 129):
        ins = [40] if n < 100 else [61, 100]
        probe = bytearray(rng.choice(b"ACGT") for _ in range(n))
        for p in ins:
            probe[p:p + 6] = b"NNNNNN"
        truth = bytes(b for b in probe if b != ord("N"))
        groups.append([(truth, None)] * 6 + [(bytes(probe), None)])
    return groups


def test_pairs_at_the_tile_edges_of_k_lg_correct(built):
    """Final alignments of 63, 64, 65, 127, 128 and 129 pairs with runs of node -1 (bases the pruned graph does not hold): pairs
    40 .. 45 inside the first tile of 64, so that the kept pairs behind them and in the next tile take their slot from the lower
    lanes' count and the carried total, and, in the longer ones, pairs 61 .. 66 across the tile edge 63 | 64 and 100 .. 105.  (A local
    alignment keeps a run only with enough matches behind it, so the runs keep a distance from the last pair.)"""
    groups = _tile_groups()
    t0 = time.time()
    res, status = _correct(groups, 1, MODELS["linear"])
    refs = _refs(groups, 1, MODELS["linear"])
    assert status.tolist() == [OK] * len(groups)
    _same(res, refs, "tiles")
    for n, r, c in zip((63, 64, 65, 127, 128, 129), refs, res):
        pairs = r[4][6]
        gaps = [k for k, (v, _) in enumerate(pairs) if v == -1]
        assert len(pairs) == n and gaps == (list(range(40, 46)) if n < 100 else list(range(61, 67)) + list(range(100, 106))), (n, len(pairs), gaps)
        assert len(c.reads[6]) == n - len(gaps) and c.reads[6] == groups[[63, 64, 65, 127, 128, 129].index(n)][0][0]
    print(f"[tile edges] alignments of 63, 64, 65, 127, 128, 129 pairs with runs of node -1 before and across the tile edge 63 | 64: "
          f"equal to the restatement, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 5. the host schedule
def test_schedule_under_the_knobs(built, monkeypatch, capfd):
    groups = _fresh(9500, 40, lo=40, hi=120, kmax=8)
    rng = random.Random(9501)
    long = bytes(rng.choice(b"ACGT") for _ in range(400))
    groups.append([(_noisy(rng, long, 0.03), None) for _ in range(3)])        # (nodes + 1) x (length + 1) cells: above 0.1 MiB each
    members = sum(len(g) for g in groups)
    scores = MODELS["linear"]
    t0 = time.time()
    free, err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: _correct(groups, 1, scores))
    j0, k0, c0, b0 = _log(err)
    assert free[1].tolist() == [OK] * len(groups) and j0 == members and k0 == 1 and b0 > 0
    refs = _refs(groups, 1, scores)
    _same(free[0], refs, "free")
    # the done line: the build's passes and two rounds' -- three per member with a forward pass, but the first member's first
    _, plain_err = _knobs(monkeypatch, capfd, {"VC_LARGE_LOG": "1"}, lambda: poa.run_batch(poa.group_batch(groups), capi.VcPoaGapParams(0, 1, *scores)))
    (a_plain, _), (a_corr, _) = _done(plain_err)[0], _done(err)[0]
    assert a_plain == members - len(groups) and a_corr == a_plain + 2 * members
    # every table regrown (labels are not kept here); a regrown group is corrected once, after the run that finishes it
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,s:10,p:6"}
    grown, err = _knobs(monkeypatch, capfd, env, lambda: _correct(groups, 1, scores))
    flags = set(",".join(re.findall(r"vc_large: regrow window=\d+ flags=(\S+)", err)).split(","))
    assert flags >= {"nodes", "edges", "aligned", "stack", "pairs"}, flags
    assert _log(err)[0] == members and _log(err)[2] == c0
    assert _flat(grown[0]) == _flat(free[0])
    # the matrix budget: a launch holds consecutive jobs while their (nodes + 1) x (length + 1) int32 fit -- one group's jobs go over
    # several launches -- and a job above the budget runs alone
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.1"}
    tight, err = _knobs(monkeypatch, capfd, env, lambda: _correct(groups, 1, scores))
    budget, launches, fill = int(0.1 * 2 ** 20) // 4, [], 0
    for g, r in zip(groups, refs):
        for s, _ in g:
            need = (r[3] + 1) * (len(s) + 1)
            if launches and fill + need <= budget:
                launches[-1].append(need); fill += need
            else:
                launches.append([need]); fill = need
    over = [l for l in launches if sum(l) > budget]
    assert len(over) == 3 and all(len(l) == 1 for l in over) and any(len(l) > 1 for l in launches) and len(launches) > len(groups)
    assert _log(err)[:3] == (members, len(launches), c0)
    assert _flat(tight[0]) == _flat(free[0])
    # several host groups, small matrices and small tables together
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_CAPS": "n:5,e:5,a:7,s:10,p:6", "VC_LARGE_ARENA_MB": "1", "VC_LARGE_MAT_MB": "0.1"}
    both, err = _knobs(monkeypatch, capfd, env, lambda: _correct(groups, 1, scores))
    assert len(re.findall(r"vc_large: group windows=", err)) >= 3 and _log(err)[0] == members and _log(err)[2] == c0
    assert _flat(both[0]) == _flat(free[0])
    print(f"[schedule] {members} members of {len(groups)} groups: 1 launch unconstrained, {len(launches)} under a 0.1 MiB matrix budget "
          f"({len(over)} of one job above it), every table regrown and the jobs counted once; results equal, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 6. statuses
def test_a_group_that_is_not_computed_beside_valid_ones(built, monkeypatch, capfd):
    """As in the tests of the other outputs, the group that is not computed is one the arena budget refuses: its members carry
    VC_WIN_OVERFLOW, score 0 and no bytes, and the rest of the batch is computed."""
    groups = _fresh(9600, 20, hi=120, kmax=8)
    rng = random.Random(9601)
    want = _correct(groups, 1, MODELS["affine"])
    big = [(bytes(rng.choice(b"ACGT") for _ in range(3000)), None) for _ in range(24)]
    g2 = groups[:7] + [big] + groups[7:]
    t0 = time.time()
    got, _ = _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: _correct(g2, 1, MODELS["affine"]))
    assert got[1].tolist() == [OK] * 7 + [capi.VC_WIN_OVERFLOW] + [OK] * 13
    c = got[0][7]
    assert c.status.tolist() == [capi.VC_WIN_OVERFLOW] * 24 and c.scores.tolist() == [0] * 24 and c.reads == [b""] * 24 and c.consensus == b""
    assert _flat(got[0][:7] + got[0][8:]) == _flat(want[0])
    with pytest.raises(poa.PoaError):
        _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: poa.poa_correct(g2, 1, gap_extend=-6))
    loose, _ = _knobs(monkeypatch, capfd, {"VC_LARGE_ARENA_MB": "4"}, lambda: poa.poa_correct(g2, 1, gap_extend=-6, strict=False))
    assert loose[7] is None and loose[0].reads == want[0][0].reads
    print(f"[statuses] a refused group's members carry its status; the rest equal to the call without it, {time.time() - t0:.1f} s")


def test_a_call_whose_jobs_are_all_empty_allocates_nothing(built, monkeypatch, capfd):
    """Every member of the call is empty, so every final graph has no node and every job is an empty alignment: the job stage lists
    its jobs and stops before its device allocation -- the log line counts the jobs and no launch, cell or byte.  (A correction job
    is empty only where the member or the graph is, so the members here cannot have bases.)  Every member is VC_WIN_OK with the
    restatement's result: the empty correction, score 0."""
    groups = [[(b"", None)] * 4, [(b"", None)] * 6, [], [(b"", None)] * 5]
    env = {"VC_LARGE_LOG": "1", "VC_LARGE_MAT_MB": "0.01", "VC_LARGE_ARENA_MB": "0.5"}
    t0 = time.time()
    for model in MODELS:
        got, err = _knobs(monkeypatch, capfd, env, lambda: _correct(groups, 1, MODELS[model]))
        assert _log(err) == (15, 0, 0, 0), err
        assert got[1].tolist() == [OK] * 4
        _same(got[0], _refs(groups, 1, MODELS[model]), ("empty", model))
    print(f"[empty jobs] 15 empty members of 4 groups, three gap models: 15 jobs, no launch, no cell, no byte copied; equal to the "
          f"restatement, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 7. calls without correction
def test_calls_without_correction_are_unchanged(built, monkeypatch, capfd):
    groups = _fresh(9700, 24, hi=150, kmax=8)
    batch = poa.group_batch(groups)
    p = capi.VcPoaGapParams(0, 1, *MODELS["convex"])
    monkeypatch.setenv("VC_LARGE_LOG", "1")

    def logged(f):
        capfd.readouterr()
        out = f()
        return out, capfd.readouterr().err
    try:
        before = [logged(f) for f in (lambda: poa.run_batch(batch, p), lambda: poa.run_batch_msa(batch, p, 7))]
        corr, err = logged(lambda: poa.run_batch_correct(batch, p, capi.VcPoaPruneParams(*DEFAULTS)))
        assert "vc_large: correct jobs=" in err
        after = [logged(f) for f in (lambda: poa.run_batch(batch, p), lambda: poa.run_batch_msa(batch, p, 7))]
    finally:
        monkeypatch.delenv("VC_LARGE_LOG")
    for (b, eb), (a, ea) in zip(before, after):
        assert "vc_large: correct" not in eb + ea and eb == ea and "vc_large: done" in eb     # the same log: the same passes and launches
    assert before[0][0][0] == after[0][0][0] == [c.consensus for c in corr[0]]
    assert [(m.rows, m.members, m.coverage.tolist()) for m in before[1][0][0]] == [(m.rows, m.members, m.coverage.tolist()) for m in after[1][0][0]]
    print("[calls without correction] vc_poa_run_gaps and vc_poa_run_msa give the same bytes and the same log lines before and after a "
          "correction call, and log no correct line")


# ------------------------------------------------------------------ 8. the haplotype window overload
def test_member_0_equals_the_window_overload_on_full_span_layers(built):
    """The existing, pinned path: vc_large_run, mode 0, on the same data given as a window -- member 0 the backbone, every other
    member a layer that spans [0, L - 1] -- at 3 / -5 / -4, global, three rounds.  All members have a quality string and the
    backbone has at least 200 bases: the overload takes a layer as spanning the window only when its end lies beyond
    L - floor(0.01 L), and refuses an end at L, so floor(0.01 L) must be at least 2 (a shorter backbone's layers go through the
    subgraph of their span, which a group does not have)."""
    groups = _fresh(9800, 40, lo=225, hi=320, kmin=3, kmax=16, quality="all")
    assert all(len(g[0][0]) >= 200 for g in groups)
    scores = (3, -5, -4, -4, -4, -4)
    t0 = time.time()
    res, status = _correct(groups, 1, scores, (0.2, 0.2, 3))
    batch = poa.group_batch(groups)
    wso = batch.win_seq_off.tolist()
    for w in range(len(groups)):
        L = len(groups[w][0][0])
        batch.seq_end[wso[w]:wso[w + 1]] = L - 1
    cons, st = large.large_consensus(batch, capi.default_params(min_confidence=0.2, min_support=0.2, num_prune=3, mode=0))
    assert status.tolist() == st.tolist() == [OK] * len(groups)
    assert [c.reads[0] for c in res] == cons
    assert sum(c.reads[0] != g[0][0] for c, g in zip(res, groups)) > 10
    print(f"[window overload] member 0 of {len(groups)} groups of 3-16 members: the haplotype window overload's bytes, {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ 9. the command line
def test_command_line(built, tmp_path):
    groups = _fresh(9900, 2, hi=120, kmax=6, quality="none")
    files = []
    for w, g in enumerate(groups):
        files.append(str(tmp_path / f"group{w}.fasta"))
        with open(files[-1], "wb") as f:
            for i, (s, _) in enumerate(g):
                f.write(b">r%d.%d\n%s\n" % (w, i, s))
    t0 = time.time()
    out = tmp_path / "corrected.fasta"
    p = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", "--correct", str(out), "--prune-rounds", "2", *files],
                       cwd=ROOT, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    plain = subprocess.run([sys.executable, "-m", "vechat_amd.poa", "-l", "1", *files], cwd=ROOT, capture_output=True, timeout=300)
    assert plain.returncode == 0 and p.stdout == plain.stdout                # the consensus output is unchanged
    want = b"".join(b">r%d.%d\n%s\n" % (w, i, r) for w, g in enumerate(groups)
                    for i, r in enumerate(PC.correct_group(g, 1, 5, -4, -8, num_prune=2)["reads"]))
    assert out.read_bytes() == want
    print(f"[command line] --correct on two group files: the restatement's records under the reads' own names, stdout unchanged, "
          f"{time.time() - t0:.1f} s")
