"""`bench.py --dump-outputs DIR` (CPU side): the dumped arrays are float32 / float64, at most 64 MB in all, the Gt rows round-trip
bit for bit to the u64 limbs the pairing batch wrote, and the sampled rows are the same from call to call."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs(tmp_path):
    bench = load_bench()
    rng = np.random.default_rng(0)
    n, nv = bench.DUMP_PAIRING_ROWS + 5, 2 * bench.DUMP_FLAG_ROWS + 3       # both larger than their samples
    gt = rng.integers(0, 1 << 63, size=(48, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    ok = (rng.random(nv) < 0.5).astype(np.uint8)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), gt, ok, 0)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["bls_all_valid.npy", "bls_verify_ok.npy", "bls_verify_ok_index.npy", "pairing_gt.npy", "pairing_gt_index.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(tmp_path / d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        runs.append(arrays)
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f
    a = runs[0]
    gi = a["pairing_gt_index.npy"].astype(np.int64)
    assert gi.shape == (bench.DUMP_PAIRING_ROWS,) and len(set(gi.tolist())) == gi.size and gi.max() < n
    assert np.array_equal(a["pairing_gt.npy"].astype(np.uint32).view(np.uint64), gt[:, gi].T)
    vi = a["bls_verify_ok_index.npy"].astype(np.int64)
    assert vi.shape == (bench.DUMP_FLAG_ROWS,) and np.array_equal(a["bls_verify_ok.npy"], ok[vi].astype(np.float32))
    assert a["bls_all_valid.npy"].tolist() == [0.0]


def test_dump_outputs_small_batch_is_whole(tmp_path):
    bench = load_bench()
    gt = np.arange(48 * 8, dtype=np.uint64).reshape(48, 8)
    bench.dump_outputs(str(tmp_path), gt, np.ones(8, np.uint8), 1)
    assert np.array_equal(np.load(tmp_path / "pairing_gt_index.npy"), np.arange(8))
    assert np.array_equal(np.load(tmp_path / "pairing_gt.npy").astype(np.uint32).view(np.uint64), gt.T)
    assert np.load(tmp_path / "bls_all_valid.npy").tolist() == [1.0]
