"""Inputs of tests/test_gpu_past_4gib.py: one [ROWS, 528] fp32 array on the device that lies just past the three lines at
which a narrow index wraps -- 2^32 bytes, 2^31 elements, 2^32 elements --, filled so that a read from a wrapped address
gives another value than the right one, and the rows a test looks at."""
import numpy as np

NV = 528
ROWS = 8134416                       # 17.18 GB: the first multiple of 16 behind row 8 134 407, which straddles 2^32 elements
P = 4093                             # the largest prime below 4096: element (r, c) holds (r * NV + c) mod P, exact in fp32
CANARY_FLOATS = 4096
LINES = (("2^32 bytes", 1 << 30), ("2^31 elements", 1 << 31), ("2^32 elements", 1 << 32))      # as element offsets
LINE_ROWS = tuple(line // NV for _name, line in LINES)       # 2 033 601, 4 067 203, 8 134 407: each straddles its line
GB = 1e9


def checked_rows(rows, lines=LINE_ROWS, seed=11):
    """the first 64 rows, the last 64, the 64 around each line that lies inside, 256 seeded others; sorted, distinct"""
    take = set(range(min(64, rows))) | set(range(max(rows - 64, 0), rows))
    for line in lines:
        take |= set(r for r in range(line - 32, line + 32) if 0 <= r < rows)
    take |= set(int(r) for r in np.random.RandomState(seed).randint(0, rows, 256))
    return np.array(sorted(take), dtype=np.int64)


def expected_rows(rows):
    """what fill() puts into the rows `rows`, computed on the host in int64"""
    rows = np.asarray(rows, dtype=np.int64)
    return ((rows[:, None] * NV + np.arange(NV, dtype=np.int64)[None, :]) % P).astype(np.float32)


def fill(x, slab=1 << 18):
    """x [rows, NV] fp32 on the device, in slabs (the int64 offsets of a slab take 1.1 GB, never those of the array)"""
    import torch
    for s in range(0, x.shape[0], slab):
        e = min(s + slab, x.shape[0])
        off = torch.arange(s * NV, e * NV, dtype=torch.int64, device=x.device)
        x[s:e] = torch.remainder(off, P).to(torch.float32).view(-1, NV)
        del off


def read_rows(x, rows):
    """rows of a device array [*, w] on the host, through slices only: consecutive rows as one copy"""
    rows = np.asarray(rows, dtype=np.int64)
    parts, i = [], 0
    while i < len(rows):
        j = i
        while j + 1 < len(rows) and rows[j + 1] == rows[j] + 1:
            j += 1
        parts.append(x[int(rows[i]):int(rows[j]) + 1].cpu().numpy())
        i = j + 1
    return np.concatenate(parts)


class Shared(object):
    """the shared array with CANARY_FLOATS floats of -1 behind it; a test that writes into it marks it dirty and the next
    reader fills it again; release() gives the memory back (the cases behind it need the room)"""

    def __init__(self):
        self.buf = None
        self.dirty = True

    def array(self):
        import torch
        if self.buf is None:
            self.buf = torch.empty(ROWS * NV + CANARY_FLOATS, dtype=torch.float32, device="cuda")
            self.dirty = True
        x = self.buf[:ROWS * NV].view(ROWS, NV)
        if self.dirty:
            fill(x)
            self.buf[ROWS * NV:] = -1.0
            torch.cuda.synchronize()
            self.dirty = False
        return x

    def canary_intact(self):
        return bool((self.buf[ROWS * NV:] == -1.0).all())

    def release(self):
        import torch
        self.buf = None
        self.dirty = True
        torch.cuda.empty_cache()
