"""utils_v2.GetTensorDevice without a GPU: the slab cutter and the merge of lines the device leaves to the host, with
the device side replaced by a stand-in that marks EVERY line HOST and copies nothing (the worst case of the fallback).
The batches must be GetTensor's -- rows bit for bit, positions, malformed lines reported, one final endFlag."""
import gzip
import os
import re
import types

import numpy as np
import pytest

import textparse_cases as T


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("textparse")
    out = {}
    for name, text in (("golden_a", T.golden_text("a")), ("golden_b", T.golden_text("b")),
                       ("off_format", T.off_format_text()[0]), ("volume", T.volume_text(2000)),
                       ("blank_then_rows", T.blank_then_rows_text())):
        out[name] = str(d / (name + ".txt"))
        open(out[name], "wb").write(text)
    out["golden_a_gz"] = os.path.join(T.GOLD, "gettensor_a.txt.gz")
    out["volume_gz"] = str(d / "volume.txt.gz")
    with gzip.open(out["volume_gz"], "wb", compresslevel=1) as fh:
        fh.write(T.volume_text(2000))
    out["volume_nonl"] = str(d / "volume_nonl.txt")
    open(out["volume_nonl"], "wb").write(T.volume_text(2000)[:-1])
    return out


def _bad_reported(capsys):
    return sum(int(k) for k in re.findall(r"UnpackATensorRecord Failure \((\d+) malformed", capsys.readouterr().err))


def _same_batches(fn, num, monkeypatch, capsys, slab=None):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_TextSlabDevice", T.AllHostDevice)
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    capsys.readouterr()
    want = T.collect(utils_v2.GetTensor(fn, num, log=False))
    bad_want = _bad_reported(capsys)
    got = T.collect(utils_v2.GetTensorDevice(fn, num, "cpu", log=False))
    bad_got = _bad_reported(capsys)
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert bad_got == bad_want
    assert got[2][-1] == 1 and not any(got[2][:-1])
    return got, bad_got


@pytest.mark.parametrize("name", ["golden_a", "golden_b", "golden_a_gz"])
def test_goldens_through_the_fallback(files, name, monkeypatch, capsys):
    got, _bad = _same_batches(files[name], 16, monkeypatch, capsys)
    d = np.load(os.path.join(T.GOLD, "gettensor_%s.npz" % name[7]), allow_pickle=True)
    assert np.array_equal(got[0], np.ascontiguousarray(d["X"], dtype=np.float32).reshape(-1, T.NV).view(np.uint32))
    assert [b":".join((c, p, s.upper())).decode() for c, p, s in got[1]] == [str(p) for p in d["pos"]]


def test_off_format_lines_through_the_fallback(files, monkeypatch, capsys):
    got, bad = _same_batches(files["off_format"], 50, monkeypatch, capsys)
    assert bad > 10 and len(got[1]) > 50


@pytest.mark.parametrize("name", ["volume", "volume_gz", "volume_nonl", "blank_then_rows"])
@pytest.mark.parametrize("slab", [None, 4096, 65536, 1 << 20])
def test_slab_cuts_through_the_fallback(files, name, slab, monkeypatch, capsys):
    got, _bad = _same_batches(files[name], 300, monkeypatch, capsys, slab)
    assert sum(got[3]) == len(got[1]) > 250


def test_stream_form_of_a_plain_file(files, monkeypatch, capsys):
    monkeypatch.setenv("CV_TEXT", "stream")
    _same_batches(files["volume_nonl"], 700, monkeypatch, capsys, 65536)


def test_device_parser_without_a_gpu_is_an_error(files, monkeypatch):
    """CV_TEXT_PARSE=device on a box without a GPU: the model's usual error, no silent host parse"""
    import torch
    from clairvoyante_amd import _lib, callVar, utils_v2
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    assert callVar.parses_on_device(files["volume"])
    with pytest.raises(_lib.CvError, match="needs an AMD GPU"):
        next(utils_v2.GetTensorDevice(files["volume"], 100, "cuda", log=False))
    a = types.SimpleNamespace(tensor_fn=files["volume"], chkpnt_fn="none", call_fn=os.devnull, qual=None, sampleName="S",
                              ref_fn=None, threads=None, showRef=False, v3=True, v2=False, slim=False)
    with pytest.raises(_lib.CvError, match="needs an AMD GPU"):
        callVar.Run(a)


def test_parser_choice_follows_the_input(files, monkeypatch):
    from clairvoyante_amd import callVar
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    assert not callVar.parses_on_device("PIPE")
    monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (1, None))       # None: never for that form
    assert callVar.parses_on_device(files["volume"]) and not callVar.parses_on_device(files["volume_gz"])
    monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (os.path.getsize(files["volume"]), os.path.getsize(files["volume_gz"]) + 1))
    assert callVar.parses_on_device(files["volume"]) and not callVar.parses_on_device(files["volume_gz"])
    assert not callVar.parses_on_device(files["golden_a"])
    monkeypatch.setenv("CV_TEXT_PARSE", "host")
    assert not callVar.parses_on_device(files["volume"])
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    assert callVar.parses_on_device(files["golden_a"]) and not callVar.parses_on_device("PIPE")
