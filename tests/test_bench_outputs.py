"""CPU test of bench.py --dump-outputs: what is written, in which types, within 64 MB, and the same rows for the same batch."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _outputs(B):
    g = torch.Generator().manual_seed(5)
    return {"shuffled_decks": torch.randint(0, 256, (B, 6656), dtype=torch.uint8, generator=g),
            "proofs": torch.randint(0, 256, (B, 6368), dtype=torch.uint8, generator=g),
            "prove_status": torch.zeros(B, dtype=torch.int32), "verify_status": torch.arange(B, dtype=torch.int32) % 5}


def _load(d, prefix=""):
    return {f[len(prefix):-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.startswith(prefix) and f.endswith(".npy")}


def test_small_batch_is_written_whole(tmp_path):
    import bench
    arrays = _outputs(40)
    rows = bench.write_outputs(str(tmp_path), arrays)
    got = _load(str(tmp_path))
    assert sorted(got) == ["proofs", "prove_status", "rows", "shuffled_decks", "verify_status"]
    assert list(rows) == list(range(40)) and np.array_equal(got["rows"], np.arange(40, dtype=np.float64))
    assert got["shuffled_decks"].dtype == np.float32 and got["verify_status"].dtype == np.float64
    for name, t in arrays.items():
        assert np.array_equal(got[name], t.numpy().astype(got[name].dtype)), name


def test_large_batch_is_a_fixed_sample_below_64_mb(tmp_path):
    import bench
    B = 262144
    arrays = _outputs(B)
    a, b = tmp_path / "a", tmp_path / "b"
    rows = bench.write_outputs(str(a), arrays, prefix="rank1_")
    assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 10**6
    got = _load(str(a), "rank1_")
    idx = torch.from_numpy(rows)
    for name, t in arrays.items():
        assert np.array_equal(got[name], t[idx].numpy().astype(got[name].dtype)), name
    assert np.array_equal(bench.write_outputs(str(b), arrays, prefix="rank1_"), rows)      # same batch, same rows
