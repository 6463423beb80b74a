"""bench.py --dump-outputs on the host: the film as the timed path returns it, and over the size cap a fixed, seeded pixel sample of it."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Film:
    """Stands in for a Context: the two film read-backs dump_outputs() calls."""
    def __init__(self, h, w):
        rng = np.random.default_rng(5)
        self.xyzw = rng.random((h, w, 4), dtype=np.float32)
        self.rgb = rng.random((h, w, 3), dtype=np.float32)

    def film_xyzw(self):
        return self.xyzw.copy()

    def film_rgb(self):
        return self.rgb.copy()


def test_dump_outputs_writes_the_whole_film(tmp_path):
    f = _Film(64, 48)
    _bench().dump_outputs(f, str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ["film_rgb.npy", "film_xyzw.npy"]
    assert np.array_equal(np.load(str(tmp_path / "film_xyzw.npy")), f.xyzw)
    assert np.array_equal(np.load(str(tmp_path / "film_rgb.npy")), f.rgb)


def test_dump_outputs_samples_a_film_over_the_cap(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BYTES", 1 << 20)
    f = _Film(512, 512)                                   # 7 MB of film
    for run in ("a", "b"):
        b.dump_outputs(f, str(tmp_path / run))
    names = ["film_pixel_index.npy", "film_rgb.npy", "film_xyzw.npy"]
    assert sorted(os.listdir(str(tmp_path / "a"))) == names
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in names) <= 1 << 20
    idx_f = np.load(str(tmp_path / "a" / "film_pixel_index.npy"))
    assert idx_f.dtype == np.float64
    idx = idx_f.astype(np.int64)
    assert len(idx) > 20000 and np.all(np.diff(idx) > 0) and idx[-1] < 512 * 512
    assert np.array_equal(np.load(str(tmp_path / "a" / "film_xyzw.npy")), f.xyzw.reshape(-1, 4)[idx])
    assert np.array_equal(np.load(str(tmp_path / "a" / "film_rgb.npy")), f.rgb.reshape(-1, 3)[idx])
    for n in names:                                       # the same sample on every run
        assert np.array_equal(np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n)))
