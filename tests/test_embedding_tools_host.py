"""Host side of getEmbedding and getTensorAndLayerPNG (no GPU: the model is a mock whose embeddings / layers return
known arrays): file names and places, the label lines pinned to the reference's get_labels
(tests/golden/embedding_labels.json, written by tests/golden/make_golden_embedding_labels.py), the checkpoint bundle,
the projector config text, and what the plot functions are handed."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HEADS = ((0, 4), (4, 6), (6, 10), (10, 16))


class EmbeddingMock(object):
    """embeddings(X) -> four arrays that depend on the rows they were asked for"""

    def __init__(self):
        self.calls = []

    def embeddings(self, X):
        X = np.asarray(X)
        self.calls.append(X.shape)
        n = X.shape[0]
        rng = np.random.RandomState(n)
        out = rng.standard_normal((n, 16)).astype(np.float32)
        out[:, 0] = X.reshape(n, -1)[:, 5]                  # (tied to the input rows)
        self.last = out
        return tuple(out[:, lo:hi] for lo, hi in HEADS)


class ArrayUtils(object):
    """DecompressArray over plain arrays (the clipping of utils_v2.py:189-207)"""

    @staticmethod
    def DecompressArray(array, start, num, maximum):
        end = 0
        if start + num >= maximum:
            num = maximum - start; end = 1
        return array[start:start + num], num, end


def _run_main(mod, monkeypatch, argv):
    monkeypatch.setattr("sys.argv", argv)
    mod.main()


@pytest.mark.parametrize("count,trailing", [(7, ""), (100000, "/")])
def test_get_embedding_over_the_mini_set(tmp_path, monkeypatch, count, trailing):
    from clairvoyante_amd import getEmbedding, tf_checkpoint, utils_v2
    binfn = os.path.join(G, "mini.bin")
    total, XC, YC, posC = utils_v2.LoadBin(binfn)
    mock = EmbeddingMock()
    monkeypatch.setattr(getEmbedding, "prepare_data", lambda args: (mock, utils_v2, total, XC, YC, posC))
    olog = str(tmp_path / "logs" / "run1") + trailing
    _run_main(getEmbedding, monkeypatch, ["getEmbedding.py", "--bin_fn", binfn, "--chkpnt_fn", "unused", "--olog_dir", olog,
                                          "--count", str(count)])
    n = min(count, total)                                    # --count above total clips
    assert mock.calls == [(n, 33, 4, 4)]
    X, _, _ = utils_v2.DecompressArray(XC, 0, n, total)
    Y, _, _ = utils_v2.DecompressArray(YC, 0, n, total)
    assert np.array_equal(mock.last[:, 0], np.asarray(X, dtype=np.float32).reshape(n, -1)[:, 5])
    # the four metadata files one level down, OLOG/<basename of OLOG>/NAME.tsv (write_metadata :44-53)
    labels = getEmbedding.get_labels(np.asarray(Y))
    assert len(labels[0]) == n + 1 and labels[0][0] == "A\tC\tG\tT"
    for name, lab in zip(getEmbedding.VARIABLES, labels):
        path = os.path.join(str(tmp_path / "logs" / "run1"), "run1", name + ".tsv")
        assert open(path).read() == "".join(l + "\n" for l in lab)
        assert not os.path.exists(os.path.join(str(tmp_path / "logs" / "run1"), name + ".tsv"))
    # the checkpoint: four float32 variables, by name, shape and bits
    got = tf_checkpoint.read_bundle(os.path.join(olog, "model.ckpt-1"))
    assert sorted(got) == ["BaseChange", "IndelLength", "VarType", "Zygosity"]
    for name, (lo, hi) in zip(getEmbedding.VARIABLES, HEADS):
        assert got[name].dtype == np.float32 and got[name].shape == (n, hi - lo)
        assert np.array_equal(got[name].view(np.uint32), np.ascontiguousarray(mock.last[:, lo:hi]).view(np.uint32))
    for ext in (".index", ".data-00000-of-00001"):
        assert os.path.exists(os.path.join(olog, "model.ckpt-1" + ext))
    assert open(os.path.join(olog, "checkpoint")).read() == \
        'model_checkpoint_path: "model.ckpt-1"\nall_model_checkpoint_paths: "model.ckpt-1"\n'
    # the projector config: exact text, paths as os.path.join(olog_dir, NAME.tsv)
    want = "".join('embeddings {\n  tensor_name: "%s:0"\n  metadata_path: "%s"\n}\n' % (v, os.path.join(olog, v + ".tsv"))
                   for v in ("BaseChange", "Zygosity", "VarType", "IndelLength"))
    assert open(os.path.join(olog, "projector_config.pbtxt")).read() == want


def test_label_lines_are_the_reference_get_labels(tmp_path):
    from clairvoyante_amd import getEmbedding
    fx = json.load(open(os.path.join(G, "embedding_labels.json")))
    y = np.asarray(fx["y"], dtype=np.float64)
    assert y.shape == (40, 16) and (y != 0).any(axis=0).all() and ((y[:, 4] == 0.5) & (y[:, 5] == 0.5)).any()
    got = getEmbedding.get_labels(y)
    for name, lab in zip(getEmbedding.VARIABLES, got):
        assert lab == fx[name], name
    assert len(fx["Zygosity"]) < 40                          # a 0.5 / 0.5 row gives no zygosity line
    # ... and through the files
    olog = str(tmp_path / "o")
    x = np.zeros((40, 33, 4, 4), dtype=np.float32)
    getEmbedding.visualize_embedding(None, EmbeddingMock(), ArrayUtils, 40, x, y, olog, 10000)
    for name in getEmbedding.VARIABLES:
        assert open(os.path.join(olog, "o", name + ".tsv")).read().split("\n")[:-1] == fx[name]


def test_projector_config_escapes_like_the_text_format():
    from clairvoyante_amd import getEmbedding
    text = getEmbedding.projector_config('a "b"\\c')
    assert 'metadata_path: "a \\"b\\"\\\\c/BaseChange.tsv"' in text


class LayersMock(object):
    def __init__(self, arch="slim"):
        c = {"slim": ((33, 8), (33, 16), (33, 32), 36, 18), "tiny": ((33, 8), (29, 8), (26, 8), 36, 18), "full": ((33, 16), (29, 32), (26, 48), 336, 168)}[arch]
        self.c = c
        self.calls = []
        self.returned = []

    def layers(self, X, names):
        n = np.asarray(X).shape[0]
        self.calls.append((n, tuple(names)))
        rng = np.random.RandomState(len(self.calls))
        shp = {"conv1": (n, self.c[0][0], 4, self.c[0][1]), "conv2": (n, self.c[1][0], 4, self.c[1][1]),
               "conv3": (n, self.c[2][0], 4, self.c[2][1]), "fc4": (n, self.c[3]), "fc5": (n, self.c[4]),
               "YBaseChangeSigmoid": (n, 4), "YZygositySoftmax": (n, 2), "YVarTypeSoftmax": (n, 4), "YIndelLengthSoftmax": (n, 6)}
        d = {k: rng.standard_normal(shp[k]).astype(np.float32) for k in names}
        self.returned.append(d)
        return d


def _candidates(n):
    rng = np.random.RandomState(4)
    x = rng.randint(-40, 50, size=(n, 33, 4, 4)).astype(np.float32)
    y = np.zeros((n, 16)); y[:, 0] = 1; y[:, 4] = 1; y[:, 7] = 1; y[:, 10] = 1
    pos = np.array(["chr%d:%d:ACGTACGTACGTACGTACGTACGTACGTACGTA" % (i + 1, 1000 + i) for i in range(n)])
    return x, y, pos


def test_png_tool_hands_the_layers_to_the_plot_functions(tmp_path, monkeypatch):
    from clairvoyante_amd import getTensorAndLayerPNG as T
    x, y, pos = _candidates(3)
    mock = LayersMock("full")
    seen = []
    for fn in ("PlotTensor", "PlotFiltersConv", "PlotFiltersFC", "PlotOutputArray"):
        monkeypatch.setattr(T, fn, (lambda name: lambda ofn, *a: seen.append((name, ofn, a)))(fn))
    monkeypatch.chdir(tmp_path)
    T.CreatePNGs(None, mock, ArrayUtils, 3, x, y, pos, block=2)
    assert mock.calls == [(2, T.LAYERS), (1, T.LAYERS)]                 # a block of candidates per pass
    assert sorted(os.listdir(str(tmp_path))) == ["chr%d-%d-ACGTACGTACGTACGTACGTACGTACGTACGTA" % (i + 1, 1000 + i) for i in range(3)]
    assert [(s[0], s[1]) for s in seen] == [
        (f, "chr%d-%d-ACGTACGTACGTACGTACGTACGTACGTACGTA/%s.png" % (i + 1, 1000 + i, stem)) for i in range(3) for f, stem in
        (("PlotTensor", "tensor"), ("PlotFiltersConv", "conv1"), ("PlotFiltersConv", "conv2"), ("PlotFiltersConv", "conv3"),
         ("PlotFiltersFC", "fc4"), ("PlotFiltersFC", "fc5"), ("PlotOutputArray", "output"))]
    sizes = {"conv1": (1, 8, 9, 5, 5, 8), "conv2": (1, 8, 18, 6, 6, 9), "conv3": (1, 8, 24, 7, 7, 10),
             "fc4": (10, 16, 1, 9, 9, 10), "fc5": (10, 4, 1, 4, 4, 5)}            # the reference's call arguments (:123-146)
    for k, (name, ofn, a) in enumerate(seen):
        i = k // 7
        d = mock.returned[i // 2]; j = i % 2
        stem = os.path.basename(ofn)[:-4]
        if stem == "tensor":
            assert a[0].shape == (1, 33, 4, 4) and np.array_equal(a[0][0], x[i])
        elif stem == "output":
            assert np.array_equal(a[0], np.concatenate([d[n][j:j + 1] for n in T.LAYERS[5:]], axis=1)) and a[0].shape == (1, 16)
            assert np.array_equal(a[1], y[i].reshape(1, -1))
            assert a[2:] == (1, 4, 2, 4, 4, 5)
        else:
            assert np.array_equal(a[0], d[stem][j:j + 1]) and a[0].shape[0] == 1
            assert a[1:] == sizes[stem]


def test_png_tool_prints_the_plotting_line(tmp_path, monkeypatch, capsys):
    from clairvoyante_amd import getTensorAndLayerPNG as T
    x, y, pos = _candidates(1)
    for fn in ("PlotTensor", "PlotFiltersConv", "PlotFiltersFC", "PlotOutputArray"):
        monkeypatch.setattr(T, fn, lambda *a: None)
    monkeypatch.chdir(tmp_path)
    T.CreatePNGs(None, LayersMock(), ArrayUtils, 1, x, y, pos)
    assert capsys.readouterr().err == "Plotting chr1-1000-ACGTACGTACGTACGTACGTACGTACGTACGTA...\n"


def test_png_tool_writes_pictures_that_open(tmp_path, monkeypatch):
    pytest.importorskip("matplotlib")
    Image = pytest.importorskip("PIL.Image")
    from clairvoyante_amd import getTensorAndLayerPNG as T
    x, y, pos = _candidates(1)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(T, "DPI", 40)                         # (300 in the program: seconds per picture)
    T.CreatePNGs(None, LayersMock("tiny"), ArrayUtils, 1, x, y, pos)       # (8 filters per layer: one row of subplots each)
    d = str(tmp_path / "chr1-1000-ACGTACGTACGTACGTACGTACGTACGTACGTA")
    assert sorted(os.listdir(d)) == ["conv1.png", "conv2.png", "conv3.png", "fc4.png", "fc5.png", "output.png", "tensor.png"]
    for f in os.listdir(d):
        with Image.open(os.path.join(d, f)) as im:
            assert im.format == "PNG" and im.size[0] > 50 and im.size[1] > 10


def test_missing_matplotlib_is_named(monkeypatch):
    import builtins
    from clairvoyante_amd import getTensorAndLayerPNG as T
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(SystemExit, match="matplotlib"):
        T.PlotTensor("x.png", np.zeros((1, 33, 4, 4), dtype=np.float32))


@pytest.mark.parametrize("name", ["getEmbedding", "getTensorAndLayerPNG"])
def test_no_arguments_print_help_and_exit_1(name, monkeypatch, capsys):
    import importlib
    mod = importlib.import_module("clairvoyante_amd." + name)
    monkeypatch.setattr("sys.argv", [name + ".py"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert "usage:" in out and "--chkpnt_fn" in out and "--slim" in out


def test_get_embedding_without_olog_dir_exits_with_a_message(monkeypatch):
    from clairvoyante_amd import getEmbedding
    monkeypatch.setattr("sys.argv", ["getEmbedding.py", "--bin_fn", "x.bin"])
    with pytest.raises(SystemExit, match="--olog_dir"):
        getEmbedding.main()


def test_get_embedding_flags_and_defaults(monkeypatch):
    from clairvoyante_amd import getEmbedding
    monkeypatch.setattr("sys.argv", ["getEmbedding.py", "--olog_dir", "o"])
    a = getEmbedding.get_arguements()
    assert (a.bin_fn, a.tensor_fn, a.var_fn, a.bed_fn, a.chkpnt_fn, a.olog_dir, a.slim, a.count) == \
        (None, "vartensors", "truthvars", None, None, "o", False, 10000)


def test_both_programs_are_submodules_now():
    from clairvoyante_amd import __main__ as entry
    for n in ("getEmbedding", "getTensorAndLayerPNG"):
        assert n in entry.SUBMODULES and n not in entry.NOT_BUILT
    assert entry.NOT_BUILT == ("demoRun",)
