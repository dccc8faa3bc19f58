"""``bench.py --dump-outputs``: the arrays go to DIR/<name>.npy as float32 within 64 MB in all, and an array too large for
that is written as a sample whose elements depend on its size alone, so that two runs or two builds compare element for
element."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def test_dump_is_float32_within_budget_and_samples_the_same_elements(tmp_path):
    rng = np.random.default_rng(7)
    big = rng.standard_normal(16_000_000).astype(np.float32)  # ~ the parameter count; < 2^24, so indices fit float32
    arrays = {"loss_total": np.float32(1.5), "postnet_output": rng.standard_normal((4, 100, 80)),
              "parameters": big, "gradient": big * 2}
    n = bench.write_outputs(arrays, tmp_path / "a")
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(arrays) and all(a.dtype == np.float32 for a in got.values())
    assert n == sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert got["loss_total"].shape == () and float(got["loss_total"]) == 1.5
    np.testing.assert_array_equal(got["postnet_output"], arrays["postnet_output"].astype(np.float32))  # small: whole
    assert got["parameters"].size == 1 << 21
    np.testing.assert_array_equal(got["gradient"], 2 * got["parameters"])  # same size -> same elements
    assert np.isin(got["parameters"], big).all()
    # same sizes, other contents: the same positions are sampled
    bench.write_outputs({"parameters": np.arange(big.size, dtype=np.float32)}, tmp_path / "b")
    idx = np.load(tmp_path / "b" / "parameters.npy").astype(np.int64)
    assert (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(got["parameters"], big[idx])
    # more large arrays than the budget holds at 2^21 elements each: the cap halves
    many = {f"x{i}": big for i in range(9)}
    assert bench.write_outputs(many, tmp_path / "c") <= bench.DUMP_BUDGET_BYTES
    assert np.load(tmp_path / "c" / "x0.npy").size == 1 << 20
