"""bench.py --dump-outputs: what the timed path delivered, as float32 .npy files of at most 64 MB in all, for the same windows
whatever the outputs are (the sample depends on the window count and --length only); and the options a plain run parses."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = {"lengths", "status", "windows", "consensus", "consensus_windows"}


def _outputs(n, length, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(length - 40, length + 40, size=n)
    cons = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(lens.sum()))
    status = rng.integers(0, 3, size=n).astype(np.uint8)
    return torch.from_numpy(cons), torch.from_numpy(lens), status


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_dump_holds_every_window_when_small(tmp_path):
    cons, lens, status = _outputs(300, 120, 1)
    bench.dump_outputs(str(tmp_path), cons, lens, status, 120)
    f = _load(str(tmp_path))
    assert set(f) == NAMES and all(v.dtype == np.float32 for v in f.values())
    assert (f["lengths"] == lens.numpy()).all() and (f["status"] == status).all() and (f["windows"] == np.arange(300)).all()
    off = np.concatenate([[0], np.cumsum(lens.numpy())])
    assert (f["consensus_windows"] == np.arange(300)).all()
    for w, row in enumerate(f["consensus"]):
        k = int(lens[w])
        assert row[:k].astype(np.uint8).tobytes() == cons.numpy()[off[w]:off[w + 1]].tobytes()
        assert (row[k:] == -1).all()


def test_dump_of_a_large_output_is_a_fixed_sample_under_64_mb(tmp_path):
    n, length = 100000, 500
    a, b = tmp_path / "a", tmp_path / "b"
    cons, lens, status = _outputs(n, length, 2)
    bench.dump_outputs(str(a), cons, lens, status, length)
    cons2, lens2, status2 = _outputs(n, length, 3)          # other outputs of the same shape: the same windows are sampled
    bench.dump_outputs(str(b), cons2, lens2, status2, length)
    fa, fb = _load(str(a)), _load(str(b))
    assert sum(os.path.getsize(os.path.join(a, x)) for x in os.listdir(a)) <= 64 << 20
    assert 0 < len(fa["consensus_windows"]) < n and (fa["consensus_windows"] == fb["consensus_windows"]).all()
    assert fa["lengths"].size == n
    off = np.concatenate([[0], np.cumsum(lens.numpy())])
    for w, row in list(zip(fa["consensus_windows"].astype(np.int64), fa["consensus"]))[::997]:
        k = int(lens[w])
        assert row[:k].astype(np.uint8).tobytes() == cons.numpy()[off[w]:off[w + 1]].tobytes() and (row[k:] == -1).all()


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr
