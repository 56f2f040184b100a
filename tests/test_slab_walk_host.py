"""The slab walk both device line readers share (utils_v2._SlabWalk with utils_v2._while_table_full) and the contig
registry (utils_v2._ContigIds), without a GPU: the walk runs over "cpu" tensors, plain files and in-memory pieces, with a
stand-in for the line pass that consumes the complete lines of its window (k at the most per pass) and records them."""
import random

import numpy as np
import pytest
import torch

from clairvoyante_amd import _lib, utils_v2

SLABS = (1, 7, 64, 257)
LIMITS = (1, 3, None)
# (pad_always, join_unbroken, whole_lines): the truth reader's rules, the item walk's, and the item walk's padding alone
RULES = {"truth": (True, False, False), "items": (False, True, True), "items-padding": (False, False, False)}


def _random_lines(final_newline):
    rng = random.Random(5)
    rows = [bytes(rng.choice(b"abcdefgh \t0123456789") for _ in range(rng.randint(1, 40))) for _ in range(50)]
    return b"\n".join(rows) + (b"\n" if final_newline else b"")


FILES = {
    "empty": b"",
    "newline": b"\n",
    "unterminated": b"chr1 12 x",
    "long": b"a" * (4 * 257 + 30) + b"\nshort\n",          # longer than four slabs of every size
    "random": _random_lines(True),
    "random-unterminated": _random_lines(False),
}
# pieces that end exactly before and exactly after a newline
SPLIT = (b"ab 1", b"\ncd 2\n", b"ef 3\n", b"gh", b" 4", b"\n", b"\nij 5")


class _Pieces(object):
    """the chunks of a walk as a generator that records its close()"""

    def __init__(self, pieces):
        self.it = iter([("host", np.frombuffer(p, dtype=np.uint8)) for p in pieces])
        self.closed = False

    def __iter__(self):
        return self

    def __next__(self):
        if self.closed:
            raise StopIteration
        return next(self.it)

    def close(self):
        self.closed = True


class _Boom(Exception):
    def __init__(self, at):
        Exception.__init__(self)
        self.at = at


class _Stop(BaseException):
    pass


class _Pass(object):
    """the stand-in line pass: every complete line of the window, k at the most; fail_at: the line to raise _Boom at"""

    def __init__(self, k, fail_at=None, exc=_Boom):
        self.k, self.fail_at, self.exc = k, fail_at, exc
        self.got, self.padded, self.lines = [], set(), 0
        self.buf, self.next_at = None, 0

    def consume(self, buf, lo, hi, padded_end):
        if buf is not self.buf:
            self.buf, self.next_at = buf, 0
        self.padded.add(padded_end)

        def line_pass(at, n, max_lines):
            assert at == self.next_at                        # no byte twice, none left out
            text = bytes(buf[at:at + n].numpy().tobytes())
            used = lines = 0
            while lines < max_lines and text.find(b"\n", used) >= 0:
                if self.lines == self.fail_at:
                    self.got.append((text[:used], False))
                    raise self.exc(at + used)
                used = text.find(b"\n", used) + 1
                lines += 1
                self.lines += 1
            if used:
                self.got.append((text[:used], at + used == padded_end))
            self.next_at = at + used
            return used, lines

        return utils_v2._while_table_full(lo, hi, lambda n: self.k if self.k is not None else n + 1, line_pass)


def _walk(chunks, slab, rules, keep_open=()):
    def no_bgzf(piece, head):
        raise AssertionError("no BGZF piece here")
    pad_always, join_unbroken, whole_lines = RULES[rules]
    return utils_v2._SlabWalk(torch, torch.device("cpu"), chunks, slab, no_bgzf, pad_always=pad_always,
                              join_unbroken=join_unbroken, whole_lines=whole_lines, keep_open=keep_open)


def _expected(data, rules):
    """(the bytes the passes see, "the walk appended a newline")"""
    if RULES[rules][0]:
        return (data + b"\n", True) if data else (b"", False)
    adds = bool(data) and not data.endswith(b"\n")
    return data + (b"\n" if adds else b""), adds


def _check(chunks, data, slab, k, rules):
    p = _Pass(k)
    _walk(chunks, slab, rules).run(p.consume)
    want, adds = _expected(data, rules)
    assert b"".join(w for w, _last in p.got) == want
    assert all(w.endswith(b"\n") for w, _last in p.got)
    # padded_end is reported exactly when a newline was appended, and it is the offset behind that newline
    assert (p.padded - {None} != set()) == adds
    assert [last for _w, last in p.got].count(True) == int(adds) and (not adds or p.got[-1][1])


@pytest.mark.parametrize("rules", sorted(RULES))
@pytest.mark.parametrize("k", LIMITS)
@pytest.mark.parametrize("slab", SLABS)
def test_every_byte_is_handed_over_once(tmp_path, slab, k, rules):
    for name, data in sorted(FILES.items()):
        fn = str(tmp_path / name)
        with open(fn, "wb") as f:
            f.write(data)
        _check(utils_v2._truth_chunks(fn, slab), data, slab, k, rules)
    _check(_Pieces(SPLIT), b"".join(SPLIT), slab, k, rules)
    _check(_Pieces([]), b"", slab, k, rules)


@pytest.mark.parametrize("rules", sorted(RULES))
@pytest.mark.parametrize("slab", SLABS)
def test_an_aborted_pass_leaves_the_rest_of_the_file(slab, rules):
    for data in (FILES["random"], FILES["random-unterminated"], b"".join(SPLIT)):
        pieces = SPLIT if data == b"".join(SPLIT) else [data[i:i + 97] for i in range(0, len(data), 97)]
        lines = data.split(b"\n")
        for j in sorted({0, 1, len(lines) // 2, len(lines) - 2, _expected(data, rules)[0].count(b"\n") - 1}):
            chunks, p = _Pieces(pieces), _Pass(2, fail_at=j)
            walk = _walk(chunks, slab, rules, keep_open=(_Boom,))
            with pytest.raises(_Boom) as e:
                walk.run(p.consume)
            assert not chunks.closed                         # rest() continues over the chunks
            rest, more = walk.rest(e.value.at)
            assert rest + b"".join(np.asarray(piece).tobytes() for kind, piece in more if kind is not None) \
                == b"\n".join(lines[j:])
            assert b"".join(w for w, _last in p.got) == b"".join(ln + b"\n" for ln in lines[:j])


@pytest.mark.parametrize("rules", sorted(RULES))
def test_the_chunks_are_closed_unless_the_owner_continues_over_them(rules):
    chunks = _Pieces(SPLIT)
    _walk(chunks, 7, rules).run(_Pass(None).consume)
    assert chunks.closed
    for keep_open, exc, closed in (((), _Boom, True), ((_Boom,), _Boom, False), ((_Boom,), KeyError, True),
                                   ((_Boom, KeyError), KeyError, False), ((_Boom,), _Stop, True)):
        chunks = _Pieces(SPLIT)
        with pytest.raises(exc):
            _walk(chunks, 7, rules, keep_open).run(_Pass(None, fail_at=2, exc=exc).consume)
        assert chunks.closed == closed

    def breaks_off():                                       # the chunks themselves raise: nothing is left to continue over
        yield "host", np.frombuffer(b"ab 1\ncd", dtype=np.uint8)
        raise utils_v2._TruthHandOver("the stream breaks off")
    p = _Pass(None)
    with pytest.raises(utils_v2._TruthHandOver):
        _walk(breaks_off(), 7, rules).run(p.consume)
    assert p.got == []                                       # (the look-ahead: a piece passes once the next one is known)


def test_the_loop_passes_again_only_while_the_line_table_is_full():
    calls = []

    def line_pass(at, n, max_lines):
        calls.append((at, n, max_lines))
        return {0: (10, 4), 10: (6, 4), 16: (0, 0)}[at]
    assert utils_v2._while_table_full(0, 20, lambda n: 4, line_pass) == 16 and calls == [(0, 20, 4), (10, 10, 4), (16, 4, 4)]
    calls[:] = []
    assert utils_v2._while_table_full(0, 20, lambda n: n, line_pass) == 10 and calls == [(0, 20, 20)]
    assert utils_v2._while_table_full(5, 5, lambda n: 4, line_pass) == 0 and len(calls) == 1


# ---- the contig registry -------------------------------------------------------------------------------------------------
class _Refused(Exception):
    pass


OWNERS = {
    "truth": lambda: utils_v2._ContigIds(utils_v2._TruthHandOver),
    "trainset": lambda: utils_v2._ContigIds(*utils_v2._TrainsetBuilder._REFUSAL),
    "bam": lambda: utils_v2._ContigIds(*utils_v2._BamTrainsetBuilder._REFUSAL),
}
TEXTS = {    # owner -> exception, the text for a token that is refused (None: any token is taken), the text past the limit
    "truth": (utils_v2._TruthHandOver, None, "more than 3 contigs"),
    "trainset": (utils_v2._TrainsetFallback, "a contig token with ':', NUL or a byte >= 0x80", "more than 3 contigs"),
    "bam": (_lib.CvError, "GetTrainingSetFromBam: contig name %r holds ':', NUL or a byte >= 0x80",
            "GetTrainingSetFromBam: more than 3 contigs"),
}


@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_contig_ids_come_in_order_of_first_appearance(owner, monkeypatch):
    monkeypatch.setattr(utils_v2, "TRAINSET_MAX_CONTIGS", 3)
    exc, bad_text, many_text = TEXTS[owner]
    reg = OWNERS[owner]()
    assert [reg.id_of(n) for n in (b"chr2", b"chr1", b"chr2", b"chr10", b"chr1")] == [0, 1, 0, 2, 1]
    assert reg.names == [b"chr2", b"chr1", b"chr10"] and reg.ids == {b"chr2": 0, b"chr1": 1, b"chr10": 2}
    with pytest.raises(exc) as e:
        reg.id_of(b"chr3")                                   # name number TRAINSET_MAX_CONTIGS + 1
    assert str(e.value) == many_text and type(e.value) is exc
    assert reg.id_of(b"chr10") == 2 and len(reg.names) == 3  # a name it has is still answered
    for tok in (b"a:b", b"a\0b", b"caf\xc3\xa9"):
        reg = OWNERS[owner]()
        if bad_text is None:                                 # the truth reader's setting: the token check is off
            assert reg.id_of(tok) == 0 and reg.names == [tok]
            continue
        with pytest.raises(exc) as e:
            reg.id_of(tok)
        assert str(e.value) == (bad_text % (tok,) if "%r" in bad_text else bad_text) and type(e.value) is exc
        assert reg.names == [] and reg.ids == {}
    # the refusal of a token comes before the limit
    monkeypatch.setattr(utils_v2, "TRAINSET_MAX_CONTIGS", 0)
    if bad_text is not None:
        with pytest.raises(exc) as e:
            OWNERS[owner]().id_of(b"a:b")
        assert "':'" in str(e.value)


def test_a_builder_starts_from_the_names_of_its_tables():
    reg = utils_v2._ContigIds(*utils_v2._TrainsetBuilder._REFUSAL, names=[b"x", b"y"])
    assert reg.id_of(b"y") == 1 and reg.id_of(b"z") == 2 and reg.names == [b"x", b"y", b"z"]
