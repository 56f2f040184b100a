"""The corpus of c-blosc chunks shared by test_blosc_core_sanitized.py, test_blosc_plan_host.py and test_gpu_blosc.py:
chunks from both writers of the project, hand-assembled LZ4 streams at the format's edges, the committed real c-blosc
fixtures, and a seeded generator of damaged chunks.  The shapes are the smallest at which the decoder can still go
wrong, not the workload's."""
import os
import pickle
import struct

import numpy as np

from clairvoyante_amd import utils_v2

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
OK, HOST = 1, 2


# ---- LZ4 block streams by hand ------------------------------------------------------------
def _length(v):
    """the extension bytes of a length field whose nibble is 15"""
    out = bytearray()
    v -= 15
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)
    return bytes(out)


def lz4_stream(seqs):
    """[(literal bytes, match length or None, distance)] -> (stream, what it decodes to); the last sequence has no match"""
    s, raw = bytearray(), bytearray()
    for lit, ml, dist in seqs:
        tok = (min(len(lit), 15) << 4) | (min(ml - 4, 15) if ml is not None else 0)
        s.append(tok)
        if len(lit) >= 15:
            s += _length(len(lit))
        s += lit; raw += lit
        if ml is not None:
            assert 0 < dist <= len(raw) and ml >= 4
            s += struct.pack("<H", dist)
            if ml - 4 >= 15:
                s += _length(ml - 4)
            for _ in range(ml):
                raw.append(raw[-dist])
    return bytes(s), bytes(raw)


def container(nbytes, typesize, blocksize, flags, blocks):
    """a chunk from ready-made streams: blocks = [[stream of split 0, ...], ...]"""
    nb = len(blocks)
    body, starts = bytearray(), []
    for splits in blocks:
        starts.append(16 + 4 * nb + len(body))
        for st in splits:
            body += struct.pack("<i", len(st)) + st
    head = bytes([2, 1, flags, typesize]) + struct.pack("<iii", nbytes, blocksize, 16 + 4 * nb + len(body))
    return head + b"".join(struct.pack("<i", s) for s in starts) + bytes(body)


def pickled(seqs_of_body, protocol5=True):
    """one unsplit, unshuffled chunk (typesize 1) whose stream decodes to a pickle-like envelope around the body the
    sequences make: the header and trailer are literals, so find_array_payload sees a BINBYTES object of the body"""
    _s, body = lz4_stream(seqs_of_body + [(b"\x00", None, 0)])
    body = body[:-1]
    head = b"\x80\x05\x95" + b"\x00" * 8 + b"B" + struct.pack("<I", len(body)) if protocol5 else b"\x80\x02T" + struct.pack("<i", len(body))
    first = seqs_of_body[0]
    seqs = [(head + first[0], first[1], first[2])] + list(seqs_of_body[1:]) + [(b"\x94.", None, 0)]
    stream, raw = lz4_stream(seqs)
    assert raw == head + body + b"\x94."
    return container(len(raw), 1, len(raw), (1 << 5) | 0x10, [[stream]]), body


def _rng(seed):
    return np.random.RandomState(seed)


def candidates(n, seed=0):
    """X-like fp32 [n,33,4,4] (small integers, many zeros) and Y-like float64 [n,16] one-hot groups"""
    r = _rng(seed)
    x = np.zeros((n, 33, 4, 4), dtype=np.float32)
    depth = r.randint(4, 80, size=(n, 1, 1))
    ref = r.randint(0, 4, size=(n, 33))
    idx = np.arange(33)
    for i in range(n):
        x[i, idx, ref[i], 0] = depth[i, 0, 0]
        x[i, idx, ref[i], 3] = -r.binomial(3, 0.1, size=33)
    x[:, 16, :, 1] = r.randint(-5, 5, size=(n, 4))
    y = np.zeros((n, 16))
    y[np.arange(n), r.randint(0, 4, n)] = 1; y[np.arange(n), 4 + r.randint(0, 2, n)] = 1
    y[np.arange(n), 6 + r.randint(0, 4, n)] = 1; y[np.arange(n), 10 + r.randint(0, 6, n)] = 1
    return x, y


def edge_streams():
    """[(name, chunk, body or None)]: hand-assembled streams at the edges of the format"""
    out = []
    seed = bytes(range(1, 33))

    def add(name, seqs, **kw):
        chunk, body = pickled(seqs, **kw)
        out.append((name, chunk, body))
    add("run of one byte, 70 000 long", [(seed, 70000, 1)])
    add("run of one byte, 262 124 long", [(seed, 262124, 1)])
    for period in range(2, 16):
        add("period %d, match of 300" % period, [(seed, 300, period), (b"xy", 4 + period, period)])
    for ln in (15, 15 + 255, 15 + 2 * 255, 14, 16, 15 + 254, 15 + 256):
        add("match length field %d" % ln, [(seed, ln + 4, 20), (b"ab", 5, 3)])
        add("literal length %d" % ln, [(seed, 8, 5), (bytes(_rng(ln).randint(0, 256, ln).astype(np.uint8)), 6, 40)])
    add("literals only", [(bytes(_rng(3).randint(0, 256, 5000).astype(np.uint8)), 4, 1)])
    add("many short sequences", [(seed, 4, 7)] + [(bytes([k & 255]), 4 + k % 9, 1 + k % 30) for k in range(3000)])
    add("distance 65535", [(bytes(_rng(4).randint(0, 256, 65535).astype(np.uint8)), 100, 65535), (b"q", 66000, 65535)])
    add("protocol 2 envelope", [(seed, 40, 8)], protocol5=False)
    return out


def literal_only_chunk():
    """a chunk whose one stream is a single literal run (no pickle: the payload is not recognised by either side)"""
    data = bytes(_rng(9).randint(0, 256, 700).astype(np.uint8))
    stream, raw = lz4_stream([(data, None, 0)])
    return container(len(raw), 1, len(raw), (1 << 5) | 0x10, [[stream]])


def zero_literal_ending():
    """INVALID for the core: the last sequence holds no literal (the stream ends on a bare token behind a match)"""
    stream, raw = lz4_stream([(bytes(range(40)), 30, 8)])
    stream += b"\x00"
    return container(len(raw), 1, len(raw), (1 << 5) | 0x10, [[stream]])


def writer_chunks():
    """[(name, chunk)] from the two writers: pickled arrays in every layout the reader has a path for"""
    x, y = candidates(24, seed=1)
    out = []

    def pack(a, blocksize=None, protocol=pickle.HIGHEST_PROTOCOL):
        return utils_v2.blosc_compress(pickle.dumps(a, protocol), a.itemsize, blocksize)
    raw4 = pickle.dumps(x, pickle.HIGHEST_PROTOCOL)
    for left in (1, 3, 7568):                      # typesize 4: one split block plus a leftover block
        data = (raw4 * (1 + (8192 + left) // len(raw4)))[:8192 + left]
        out.append(("ts4 split block + leftover %d" % left, utils_v2.blosc_compress(data, 4, 8192)))
    out.append(("ts4 X, 4 KiB blocks", pack(x, 4096)))
    out.append(("ts4 X, 64 KiB blocks", pack(x, 65536)))
    out.append(("ts4 X, 1 MiB blocks (leftover only)", pack(x, 1 << 20)))
    out.append(("ts8 Y, 1 KiB blocks", pack(y, 1024)))
    out.append(("ts8 Y, 1 MiB blocks", pack(y, 1 << 20)))
    out.append(("ts1 uint8", pack(np.arange(5000, dtype=np.uint8).reshape(-1, 10), 2048)))
    out.append(("ts1 uint8 small blocks (no split)", pack(np.arange(3000, dtype=np.uint8).reshape(-1, 10), 100)))
    out.append(("dont_split X (old writer)", pack(x)))
    out.append(("dont_split Y (old writer)", pack(y)))
    out.append(("dont_split X, protocol 2", pack(x, None, 2)))
    out.append(("ts4 X, protocol 2, 4 KiB blocks", pack(x, 4096, 2)))
    noisy = x.copy()                               # one noise plane: the low mantissa byte of every element
    noisy.view(np.uint32)[...] |= _rng(5).randint(0, 256, size=x.shape).astype(np.uint32)
    out.append(("stored split (one noise plane)", pack(noisy, 16384)))
    noise = _rng(6).randint(0, 256, 4000).astype(np.uint8)
    out.append(("memcpy'd chunk (new writer)", pack(noise, 1024)))
    out.append(("memcpy'd chunk (old writer)", pack(noise)))
    out.append(("empty trailing block, old writer", pack(x[:0])))
    out.append(("empty trailing block, new writer", pack(x[:0], 65536)))
    out.append(("short last block", pack(x[:7], 4096)))
    out.append(("short last block, old writer", pack(y[:7])))
    out.append(("nbytes == 0", utils_v2.blosc_compress(b"", 4, 4096)))
    out.append(("nbytes == 0, old writer", utils_v2.blosc_compress(b"", 4)))
    return out


def fixture_chunks():
    """[(name, chunk)]: real c-blosc (lz4hc, clevel 9) chunks of the committed .bin fixtures"""
    out = []
    for fn in ("mini.bin", "mini_py2proto.bin", "cblosc_x.bin"):
        p = os.path.join(GOLDEN, fn)
        if not os.path.exists(p):
            continue
        _total, XC, YC, PC = utils_v2.LoadBin(p)
        for tag, lst in (("X", XC), ("Y", YC), ("pos", PC)):
            for k, c in enumerate(lst):
                c = c.encode("latin1") if isinstance(c, str) else bytes(c)
                out.append(("%s %s[%d]" % (fn, tag, k), c))
    return out


_corpus = None


def corpus():
    """[(name, chunk)] -- everything the device must decode itself (plan accepts, no stream comes back HOST) except
    where unsupported() says otherwise"""
    global _corpus
    if _corpus is None:
        _corpus = [(n, c) for n, c, _b in edge_streams()] + [("literal-only stream", literal_only_chunk())] + writer_chunks() \
            + fixture_chunks()
    return list(_corpus)


def unsupported(chunk):
    """a chunk cv_blosc_plan must refuse although the host decodes it: typesize not 1, 4 or 8 (position strings)"""
    return (chunk[3] or 1) not in (1, 4, 8)


NBYTES_CAP = 1 << 22       # a damaged header may claim 2 GiB: neither the tests nor the device route allocate that


def host_decompress(chunk):
    """cv_blosc_decompress's bytes, or None when it refuses (or the chunk claims more than NBYTES_CAP)"""
    if len(chunk) >= 16 and not 0 <= struct.unpack_from("<i", chunk, 4)[0] <= NBYTES_CAP:
        return None
    try:
        return utils_v2.blosc_decompress(chunk)
    except Exception:
        return None


# ---- damaged chunks -----------------------------------------------------------------------
def equal_payload_base():
    """([chunks], block_bytes): 8-candidate X blocks in every layout, all with the same payload length, so that damaged
    copies of them can stand side by side in ONE call (every chunk but the last must hold exactly block_bytes)"""
    x, _y = candidates(40, seed=13)
    chunks = [utils_v2.pack_array(x[k:k + 8], bsz) for k in range(0, 32, 8) for bsz in (None, 1024, 4096, 16384, 1 << 20)]
    return chunks, x[:8].nbytes


def mutations(count, seed, base=None):
    """`count` damaged chunks, seeded: bit flips, truncations, length words (header fields, bstarts, split sizes) rewritten"""
    r = _rng(seed)
    if base is None:
        base = [c for _n, c in corpus() if 64 < len(c) < 40000 and not unsupported(c)]
    for k in range(count):
        c = bytearray(base[r.randint(len(base))])
        kind = k % 3
        if kind == 0:
            for _ in range(r.randint(1, 5)):
                at = r.randint(len(c))
                c[at] ^= 1 << r.randint(8)
        elif kind == 1:
            c = c[:r.randint(1, len(c))]
        else:
            nblocks = max(1, -(-struct.unpack_from("<i", c, 4)[0] // max(1, struct.unpack_from("<i", c, 8)[0])))
            words = [4, 8, 12] + [16 + 4 * b for b in range(min(nblocks, 8))]
            first = struct.unpack_from("<i", c, 16)[0] if len(c) >= 20 else 0
            if 0 < first <= len(c) - 4:
                words.append(first)
            at = words[r.randint(len(words))]
            old = struct.unpack_from("<i", c, at)[0]
            new = [old + 1, old - 1, old * 2, old // 2, 0, -1, 0x7fffffff, int(r.randint(0, 1 << 20)), old + 4, old ^ (1 << r.randint(24))][r.randint(10)]
            struct.pack_into("<i", c, at, max(-(1 << 31), min(new, (1 << 31) - 1)))
        yield bytes(c)
