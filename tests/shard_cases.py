"""Inputs and helpers shared by tests/test_shard_rule_host.py and tests/test_gpu_shard_range.py: one tensor file read by
several ranks, each its own byte range (utils_v2.shard_span, GetTensor / GetTensorDevice with part=).  The device
stand-in is bgzf_cases.ZlibSlabDevice with the two things a ranged reader asks of the device on top: the newlines behind
a slab's queries (with numpy) and a handle that ends where the rank's lines end."""
import numpy as np

import bgzf_cases as B
import textparse_cases as T


class RangedZlibDevice(B.ZlibSlabDevice):
    def settle(self, up, slab, head):
        text = up[head:head + slab.n]
        out = []
        for q in slab.queries:
            hit = np.flatnonzero(text[q:] == 10)
            out.append(q + int(hit[0]) if len(hit) else slab.n)
        return np.array(out, dtype=np.int64)

    def cut(self, up, end):
        return up[:end]


def bgzf_with_empty_members(text, block):
    """`text` as BGZF members of `block` bytes with EMPTY members put in: two in front, one behind EVERY member (a cut
    falls into the DEFLATE data of some member, so the member it names -- the next one -- is an empty one), three in a
    row behind every seventh, the EOF marker at the end"""
    import zlib
    empty = B.bgzf_member(B.deflate(b""), 0, 0)
    out = [empty, empty]
    for k, at in enumerate(range(0, len(text), block)):
        piece = text[at:at + block]
        out += [B.bgzf_member(B.deflate(piece), len(piece), zlib.crc32(piece)), empty]
        if k % 7 == 6:
            out += [empty, empty]
    return b"".join(out) + empty


def parts_concatenated(reader, ws):
    """reader(rank) -> a GetTensor-like generator over part (rank, ws); -> what T.collect gives for the ranks one behind
    the other, the end flags per rank, the rows per rank"""
    xs, pos, flags, sizes = [], [], [], []
    for r in range(ws):
        x, p, f, s = T.collect(reader(r))
        xs.append(x); pos += p; flags.append(f); sizes.append(sum(s))
    return np.concatenate(xs), pos, flags, sizes


def tensor_text(x, seed=3, bad_every=97):
    """the candidates x [n,33,4,4] as a text tensor file in the producer's format (every `bad_every`-th with an N as
    its centre base: dropped by the readers) -> bytes"""
    rng = np.random.RandomState(seed)
    raw = x.copy()
    for i in range(1, 4):
        raw[:, :, :, i] += raw[:, :, :, 0]
    lines = []
    for j in range(raw.shape[0]):
        seq = "".join(rng.choice(list("ACGT"), 33))
        if j % bad_every == 5:
            seq = seq[:16] + "N" + seq[17:]
        lines.append("%s %d %s %s\n" % ("chr%d" % (1 + j % 4), 10000 + 7 * j, seq, " ".join("%0.1f" % v for v in raw[j].reshape(-1))))
    return "".join(lines).encode()
