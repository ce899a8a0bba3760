"""bench.py --dump-outputs: the arrays are written whole up to the size cap, and past it as the same seeded sample of
rows on every run (so that two builds can be compared output for output)."""
import os

import numpy

import bench


def _arrays():
    rs = numpy.random.RandomState(5)
    return {"centroids": rs.rand(16, 4).astype(numpy.float32),
            "assignments": rs.randint(0, 16, size=10000).astype(numpy.float32)}


def test_dump_writes_whole_arrays_under_the_cap(tmp_path):
    arrays = _arrays()
    bench.dump_outputs(str(tmp_path), arrays, sum(a.nbytes for a in arrays.values()))
    assert sorted(os.listdir(tmp_path)) == ["assignments.npy", "centroids.npy"]
    for name, a in arrays.items():
        got = numpy.load(str(tmp_path / (name + ".npy")))
        assert got.dtype == a.dtype and (got == a).all()


def test_dump_samples_the_same_rows_past_the_cap(tmp_path, monkeypatch):
    arrays = _arrays()
    total = sum(a.nbytes for a in arrays.values())
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 16) + total // 4)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, total)
    data = 0
    for name, a in arrays.items():
        got = numpy.load(str(tmp_path / "a" / (name + ".npy")))
        rows = numpy.load(str(tmp_path / "a" / (name + "_rows.npy")))
        assert rows.dtype == numpy.float64 and 0 < rows.size < a.shape[0]
        assert (numpy.diff(rows) > 0).all() and rows[-1] < a.shape[0]
        assert (got == a[rows.astype(numpy.int64)]).all()
        assert (got == numpy.load(str(tmp_path / "b" / (name + ".npy")))).all()
        assert (rows == numpy.load(str(tmp_path / "b" / (name + "_rows.npy")))).all()
        data += got.nbytes + rows.nbytes
    assert data <= total // 4
