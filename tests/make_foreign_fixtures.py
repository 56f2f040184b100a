"""Writes tests/golden/deflate_foreign: DEFLATE data by libdeflate (the library htslib writes BAM through), made here
through ctypes on the installed shared library.  Committed, because the library need not exist where the tests run;
tests/test_deflate_foreign_host.py regenerates the files in memory where it does and compares.

  rows_level{1,6,9,12}.deflate, bam_level{...}.deflate   raw members of text-tensor rows and of BAM record bytes
  volume300_level{6,12}.gz                                gzip files of textparse_cases.volume_text(300)
  noisy_libdeflate.bam (+ .bai)                           golden/pileup/noisy.sam, every BGZF member by libdeflate (the
                                                          levels 1, 6, 9, 12 in turn)
The expected bytes are not stored: they are whatever zlib inflates the files to."""
import ctypes
import ctypes.util
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_writer  # noqa: E402
import foreign_cases as F  # noqa: E402
import textparse_cases as T  # noqa: E402

BAM_PAYLOAD = 9001


def load():
    """the library, or None"""
    for name in (ctypes.util.find_library("deflate"), "libdeflate.so.0", "libdeflate.so"):
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
        lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
        lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
        for fn in ("libdeflate_deflate_compress", "libdeflate_gzip_compress"):
            getattr(lib, fn).restype = ctypes.c_size_t
            getattr(lib, fn).argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        return lib
    return None


def compress(lib, data, level, gzip=False):
    c = lib.libdeflate_alloc_compressor(level)
    assert c
    try:
        out = ctypes.create_string_buffer(len(data) + len(data) // 8 + 1024)
        n = (lib.libdeflate_gzip_compress if gzip else lib.libdeflate_deflate_compress)(c, bytes(data), len(data), out, len(out))
        assert n > 0
        return out.raw[:n]
    finally:
        lib.libdeflate_free_compressor(c)


def generate(lib):
    """-> {file name: bytes}"""
    out = {}
    for name, data in sorted(F.fixture_inputs().items()):
        out[name] = compress(lib, data, int(name.split("level")[1].split(".")[0]))
    for level in (6, 12):
        out["volume300_level%d.gz" % level] = compress(lib, T.volume_text(300), level, gzip=True)
    turn = [0]

    def member(data):
        turn[0] += 1
        return compress(lib, data, F.LEVELS[turn[0] % 4])
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "n.bam")
        bam_writer.write_bam(bam, F.noisy_records(), F.noisy_refs(), block_payload=BAM_PAYLOAD, compress=member)
        out["noisy_libdeflate.bam"] = open(bam, "rb").read()
        out["noisy_libdeflate.bam.bai"] = open(bam + ".bai", "rb").read()
    return out


if __name__ == "__main__":
    lib = load()
    assert lib is not None, "libdeflate is not installed"
    os.makedirs(F.FIXTURES, exist_ok=True)
    for name, data in sorted(generate(lib).items()):
        with open(os.path.join(F.FIXTURES, name), "wb") as fh:
            fh.write(data)
        print("%-28s %7d bytes" % (name, len(data)))
