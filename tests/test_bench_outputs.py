"""bench.py --dump-outputs: the last timed step's (ids, dists, counts) as
float .npy arrays, the slots the search did not write set to fixed values, a
batch too large for the size cap reduced to a fixed sample.  CPU only."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(b, k, seed=0):
    rng = np.random.default_rng(seed)
    ids = torch.from_numpy(rng.integers(0, 10_000_000, (b, k)))
    dists = torch.from_numpy(rng.random((b, k), dtype=np.float32))
    counts = torch.from_numpy(rng.integers(0, k + 1, b).astype(np.int32))
    return ids, dists, counts


def test_dump_outputs_arrays(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    ids, dists, counts = _result(37, 10)
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), (ids, dists, counts))
    assert sorted(os.listdir(out)) == ["counts.npy", "dists.npy", "ids.npy"]
    gi, gd, gc = (np.load(out / f"{n}.npy") for n in ("ids", "dists", "counts"))
    assert gi.dtype == np.float64 and gd.dtype == np.float32 and gc.dtype == np.float64
    assert gi.shape == (37, 10) and gd.shape == (37, 10) and gc.shape == (37,)
    assert np.array_equal(gc, counts.numpy())
    for q in range(37):
        c = int(counts[q])
        assert np.array_equal(gi[q, :c], ids[q, :c].numpy())
        assert np.array_equal(gd[q, :c].view(np.uint32), dists[q, :c].numpy().view(np.uint32))
        assert np.all(gi[q, c:] == -1.0) and np.all(gd[q, c:] == 0.0)


def test_dump_outputs_size_cap_takes_a_fixed_sample(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20 * (4 * 12 + 16))
    res = _result(100, 4)
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.shape == (20,) and np.all(np.diff(rows) > 0)
    total = 0
    for name in ("rows", "ids", "dists", "counts"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy"), res[2].numpy()[rows.astype(np.int64)])
