"""CPU: bench.py's --dump-outputs writer (float32 / float64 .npy files, a seeded sample of images above the size limit) and the plain / --full switch."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gswm_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_every_array_as_float32_or_float64(tmp_path):
    b = _bench()
    rng = np.random.default_rng(1)
    arrays = {"latents": rng.standard_normal((3, 4, 8, 8)).astype(np.float16), "bits": rng.integers(0, 256, (3, 32), dtype=np.uint8),
              "exact": rng.standard_normal((3, 5))}
    b.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["bits.npy", "exact.npy", "latents.npy"]
    lat, bits, exact = (np.load(tmp_path / f"{n}.npy") for n in ("latents", "bits", "exact"))
    assert lat.dtype == np.float32 and np.array_equal(lat, arrays["latents"].astype(np.float32))
    assert bits.dtype == np.float32 and np.array_equal(bits, arrays["bits"].astype(np.float32))
    assert exact.dtype == np.float64 and np.array_equal(exact, arrays["exact"])


def test_dump_over_the_limit_keeps_the_same_seeded_images(tmp_path):
    b = _bench()
    n = 64
    z = np.arange(n * 1024, dtype=np.float32).reshape(n, 1024)          # 256 KiB: image i holds i * 1024 ...
    bits = np.repeat(np.arange(n, dtype=np.float32)[:, None], 4, axis=1)
    limit = 64 * 1024 + 4096 * 2
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"z": z, "bits": bits}, limit=limit)
    za, ba = np.load(tmp_path / "a" / "z.npy"), np.load(tmp_path / "a" / "bits.npy")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    assert 0 < za.shape[0] < n and za.shape[1:] == (1024,)
    idx = za[:, 0].astype(np.int64) // 1024
    assert np.all(np.diff(idx) > 0) and np.array_equal(za, z[idx])
    assert np.array_equal(ba[:, 0].astype(np.int64), idx)                 # the same images in every array of the batch
    assert np.array_equal(za, np.load(tmp_path / "b" / "z.npy"))        # and in every run


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "out"
