"""The keyed draws (csrc/cv_draw_core.hpp through cv_draws_host) against an independent numpy restatement of
Philox4x32-10 (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
rounds), and the share stream 0 keeps at probability 0.3.  No GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = np.uint64(0xffffffff)


def philox4x32_10(key, ctr):
    """key [n,2], ctr [n,4] as uint64 arrays holding 32-bit words -> [n,4]"""
    k0, k1 = key[:, 0].copy(), key[:, 1].copy()
    c = [ctr[:, i].copy() for i in range(4)]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1)


def fnv1a32(b):
    h = 0x811c9dc5
    for x in b:
        h = ((h ^ x) * 0x01000193) % (1 << 32)
    return h


def restated(seed, stream, name, pos, late):
    pos = np.asarray(pos, dtype=np.uint64)
    n = len(pos)
    key = np.empty((n, 2), dtype=np.uint64)
    key[:, 0], key[:, 1] = seed & 0xffffffff, seed >> 32
    ctr = np.empty((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = pos & M32, pos >> np.uint64(32)
    ctr[:, 2] = np.uint64(stream) | (np.asarray(late, dtype=np.uint64) << np.uint64(8))
    ctr[:, 3] = fnv1a32(name)
    x = philox4x32_10(key, ctr)
    return (((x[:, 0] << np.uint64(32)) | x[:, 1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def test_philox_restatement_reproduces_the_published_vectors():
    """the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10): the yardstick itself is right"""
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = philox4x32_10(np.array([key], dtype=np.uint64), np.array([ctr], dtype=np.uint64))[0]
        assert tuple(int(v) for v in got) == want


def test_draws_equal_the_numpy_restatement():
    """4 096 keyed draws over both streams, positions above 2^32 and late = 1"""
    from clairvoyante_amd import draws
    rng = np.random.RandomState(5)
    assert draws.fnv1a32("ctg10") == fnv1a32(b"ctg10") and draws.fnv1a32("") == 0x811c9dc5
    n = 0
    for seed in (0, 1, 0x9e3779b97f4a7c15, (1 << 64) - 1):
        for stream in (draws.SAMPLE, draws.PAIR):
            for name in ("ctgA", "chr21"):
                pos = np.concatenate([rng.randint(1, 1 << 31, 128), (1 << 32) + rng.randint(0, 1 << 31, 64) * 7,
                                      np.array([1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3])[:64]]).astype(np.int64)
                pos = np.concatenate([pos, pos[:256 - len(pos)]])
                late = rng.randint(0, 2, len(pos)) if stream == draws.SAMPLE else np.zeros(len(pos), dtype=np.int64)
                got = draws.draws(seed, stream, name, pos, late)
                want = restated(seed, stream, name.encode(), pos, late)
                assert got.dtype == np.float64 and np.array_equal(got, want)
                assert (got >= 0).all() and (got < 1).all()
                n += len(pos)
    assert n == 4096
    # late and stream are part of the key: flipping either changes the draw
    p = np.arange(1, 257)
    a = draws.draws(9, draws.SAMPLE, "ctgA", p)
    assert not np.array_equal(a, draws.draws(9, draws.SAMPLE, "ctgA", p, np.ones(256))) and \
        not np.array_equal(a, draws.draws(9, draws.PAIR, "ctgA", p)) and not np.array_equal(a, draws.draws(9, draws.SAMPLE, "ctgB", p))
    assert np.array_equal(a, draws.draws(9, draws.SAMPLE, "ctgA", p, None))


def test_stream_0_keeps_three_tenths():
    """20 000 consecutive positions at probability 0.3: the kept share lies within four standard deviations
    (4 * sqrt(0.3 * 0.7 / 20000) = 0.013) of 0.3"""
    from clairvoyante_amd import draws
    u = draws.draws(20240613, draws.SAMPLE, "chr21", np.arange(1, 20001))
    share = float((~(u > 0.3)).mean())
    print("kept share", share)
    assert abs(share - 0.3) <= 0.013


def test_header_under_the_sanitizers(tmp_path):
    """cv_draw_core.hpp in a stand-alone program built with -fsanitize=address,undefined: same bits as the library"""
    from clairvoyante_amd import draws
    src = tmp_path / "d.cpp"
    src.write_text("""#include <stdio.h>
#include "cv_draw_core.hpp"
int main()
{
    const uint8_t n[] = "ctgA";
    const uint32_t h = cv_fnv1a32(n, 4);
    for (int64_t p = 1; p <= 64; p++)
        printf("%.17g ", cv_draw(0xfedcba9876543210ull, (int)(p & 1), h, p * 0x10000001ll, (int)(p >> 1 & 1)));
    return 0;
}
""")
    exe = str(tmp_path / "d")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "clairvoyante_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    assert out.stderr == b""
    got = [float(v) for v in out.stdout.split()]
    for p in range(1, 65):
        assert got[p - 1] == draws.draws(0xfedcba9876543210, p & 1, "ctgA", [p * 0x10000001], [p >> 1 & 1])[0]
