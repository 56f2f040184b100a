"""utils_v2.BgzfWriter(threads=N): the members of a BGZF file compressed side by side by a thread pool and written in
order.  The file is byte for byte what threads=1 (one member after the other on the caller's thread) gives -- for every
size around the 65 280-byte member boundary, compressible and random bytes, two levels, a small block, many small writes
against one large one --, cv_bgzf_scan accepts it, it inflates to its input, and a worker's exception reaches the caller."""
import gzip
import io

import numpy as np
import pytest

from clairvoyante_amd import utils_v2

SIZES = (0, 1, 65279, 65280, 65281, 1000003)
THREADS = (1, 2, 8, 16)


def _data(kind, n):
    if kind == "random":
        return np.random.RandomState(n % 1000 + 7).randint(0, 256, n, dtype=np.uint8).tobytes()
    row = b"chr1 1234567 ACGTNacgtnACGTACGTACGTACGTACGTACGTA" + b" 0.0 12.0 250.0 3.0" * 20 + b"\n"
    return (row * (n // len(row) + 1))[:n]


def _write(data, threads, pieces=None, **kw):
    out = io.BytesIO()
    w = utils_v2.BgzfWriter(out, threads=threads, **kw)
    if pieces is None:
        w.write(data)
    else:
        for at in range(0, len(data), pieces):
            w.write(data[at:at + pieces])
    w.close()
    return out.getvalue()


def _check(file, data):
    got = utils_v2.bgzf_scan(np.frombuffer(file, dtype=np.uint8))
    assert got is not None, "cv_bgzf_scan does not take the file"
    table, total = got
    assert total == len(data)
    assert gzip.decompress(file) == data


@pytest.mark.parametrize("kind", ["text", "random"])
@pytest.mark.parametrize("level", [1, 6])
def test_every_pool_size_writes_the_serial_file(kind, level):
    for n in SIZES:
        data = _data(kind, n)
        serial = _write(data, 1, level=level)
        _check(serial, data)
        for t in THREADS[1:]:
            assert _write(data, t, level=level) == serial, (n, t)


def test_small_block_and_small_writes():
    for n in (0, 1, 65281, 1000003):
        data = _data("text", n)
        serial = _write(data, 1, block=4096)
        _check(serial, data)
        for t in THREADS:
            assert _write(data, t, block=4096) == serial, (n, t)
        # many small writes against one large one: the cuts do not depend on how the bytes arrive
        whole = _write(data, 1)
        for t in THREADS:
            assert _write(data, t, pieces=997) == whole, (n, t)
            assert _write(data, t, pieces=70001) == whole, (n, t)


def test_default_pool_and_strategy(tmp_path):
    import zlib
    data = _data("text", 300000)
    fn = str(tmp_path / "t.gz")
    with utils_v2.BgzfWriter(fn) as w:                       # threads=None: min(16, usable cores)
        assert 1 <= w.threads <= 16
        w.write(data)
    file = open(fn, "rb").read()
    assert file == _write(data, 1)
    _check(file, data)
    assert _write(data, 8, strategy=zlib.Z_RLE) == _write(data, 1, strategy=zlib.Z_RLE) != file


def test_members_in_flight_are_bounded(monkeypatch):
    """at most 2 x threads members wait for the file at any time"""
    seen = []
    orig = utils_v2.BgzfWriter._put

    def put(self, data):
        orig(self, data)
        seen.append(len(self.inflight))
    monkeypatch.setattr(utils_v2.BgzfWriter, "_put", put)
    data = _data("text", 40 * 4096)
    assert _write(data, 2, block=4096) == _write(data, 1, block=4096)
    assert max(seen) == 4 and len(seen) >= 40


def test_a_workers_exception_reaches_the_caller(monkeypatch):
    calls = {"n": 0}
    orig = utils_v2.BgzfWriter.member

    def member(data, level=6, strategy=0):
        calls["n"] += 1
        if calls["n"] == 3:
            raise RuntimeError("member 3 failed")
        return orig(data, level, strategy)
    monkeypatch.setattr(utils_v2.BgzfWriter, "member", staticmethod(member))
    w = utils_v2.BgzfWriter(io.BytesIO(), threads=4, block=4096)
    with pytest.raises(RuntimeError, match="member 3 failed"):
        w.write(_data("text", 20 * 4096))
        w.close()
    w.close()                                                # whichever call raised: closing ends the pool, nothing waits
    assert w.pool is None and not w.inflight and w.fh is None
