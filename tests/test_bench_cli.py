"""bench.py's command line and --dump-outputs helpers (no GPU): --full is off by default, --steps
must be positive, the dumped arrays are float32 / float64 with every slot a caller must not read
blanked, and an array over its share of the 64 MB cap is cut to the same seeded rows every time."""
import sys

import numpy as np
import pytest

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--steps", "0")


def test_fused_arrays_blank_what_the_caller_must_not_read():
    import torch
    keys = torch.tensor([[5, 3, 9, 7], [1, 2, 99, 98]])
    fused = torch.tensor([[.4, .3, .2, .1], [.4, .3, 7., 7.]], dtype=torch.float64)
    vdist = torch.tensor([[.5, 9., .6, .7], [.1, .2, 9., 9.]])
    bscore = torch.tensor([[9., 2., 3., 9.], [4., 5., 9., 9.]], dtype=torch.float64)
    flags = torch.tensor([[1, 2, 3, 1], [3, 3, 7, 7]], dtype=torch.int32)
    n = torch.tensor([4, 2], dtype=torch.int32)
    a = bench.fused_arrays((keys, fused, vdist, bscore, flags, n))
    assert a["fused_keys"].tolist() == [[5, 3, 9, 7], [1, 2, -1, -1]]
    assert a["fused_score"].tolist() == [[.4, .3, .2, .1], [.4, .3, 0., 0.]]
    assert a["vector_distance"].dtype == np.float32
    assert np.array_equal(a["vector_distance"], np.float32([[.5, 0, .6, .7], [.1, .2, 0, 0]]))
    assert a["bm25_score"].tolist() == [[0., 2., 3., 0.], [4., 5., 0., 0.]]
    assert a["flags"].tolist() == [[1, 2, 3, 1], [3, 3, 0, 0]] and a["count"].tolist() == [4, 2]
    assert keys[1, 2] == 99                      # the step's own tensors are left alone


def test_dump_outputs_dtypes_and_cap(tmp_path, monkeypatch):
    big = np.arange(4000, dtype=np.float32).reshape(1000, 4)
    arrays = {"keys": np.array([[1, -1]], np.int64), "dist": np.float32([[.5, 0]]), "big": big}
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 3 * 1024)
    bench.dump_outputs(tmp_path / "a", arrays)
    bench.dump_outputs(tmp_path / "b", arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["big", "dist", "keys"]
    assert got["keys"].dtype == np.float64 and got["keys"].tolist() == [[1., -1.]]
    assert got["dist"].dtype == np.float32
    assert got["big"].shape == (64, 4) and sum(v.nbytes for v in got.values()) <= 3 * 1024
    rows = (got["big"][:, 0] // 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(got["big"], big[rows])
    assert np.array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
