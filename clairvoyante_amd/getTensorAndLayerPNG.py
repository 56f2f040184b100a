"""PNG pictures of the input tensor, the hidden layers and the outputs of every candidate: command line and files of
/root/reference/clairvoyante/getTensorAndLayerPNG.py (plot functions :40-108, CreatePNGs :111-146).

    python -m clairvoyante_amd.getTensorAndLayerPNG --tensor_fn TENSORS --var_fn TRUTH --chkpnt_fn MODEL [--slim]

Per candidate a directory named after its position ("chrom-coord-seq") in the working directory with tensor.png,
conv1.png, conv2.png, conv3.png (the SELU maps before pooling), fc4.png, fc5.png and output.png (predicted against
truth).  The layers are fetched for a block of candidates per pass (model.layers) and plotted one by one; the plot
functions are the reference's, with its figure sizes, tick sizes, colour maps and value ranges.  matplotlib is needed
only here and is imported when a picture is drawn.
"""
import math
import os
import sys

if __package__ in (None, ""):      # run as `python <dir>/getTensorAndLayerPNG.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
import numpy as np

LAYERS = ("conv1", "conv2", "conv3", "fc4", "fc5", "YBaseChangeSigmoid", "YZygositySoftmax", "YVarTypeSoftmax",
          "YIndelLengthSoftmax")
BLOCK = 256            # candidates per pass: 256 x (17 + 15 + 20) KB of maps of the full topology on their way to the host
DPI = 300            # of every picture (the reference's)
OUTPUT_TICKS = ["A", "C", "G", "T", "HET", "HOM", "REF", "SNP", "INS", "DEL", "0", "1", "2", "3", "4", ">4"]


def _pyplot():
    try:
        import matplotlib
    except ImportError:
        sys.exit("getTensorAndLayerPNG needs the matplotlib package, which is not installed")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return matplotlib, plt


def Prepare(args):
    """getTensorAndLayerPNG.py:11-27"""
    from . import utils_v2 as utils
    if args.slim:
        from . import clairvoyante_v3_slim as cv
    else:
        from . import clairvoyante_v3 as cv
    utils.SetupEnv()
    m = cv.Clairvoyante()
    m.init()
    m.restoreParameters(args.chkpnt_fn)
    total, XC, YC, posC = utils.GetTrainingArray(args.tensor_fn, args.var_fn, None)
    return m, utils, total, XC, YC, posC


def PlotFiltersConv(ofn, units, interval=1, xsize=18, ysize=20, xts=1, yts=1, lts=2):
    matplotlib, plt = _pyplot()
    matplotlib.rc('xtick', labelsize=xts)
    matplotlib.rc('ytick', labelsize=yts)
    matplotlib.rc('axes', titlesize=lts)
    filters = units.shape[3]
    xlen = units.shape[2]
    plot = plt.figure(1, figsize=(xsize, ysize))
    nColumns = 8
    nRows = int(math.ceil(filters / nColumns)) + 1
    for i in range(filters):
        plt.subplot(nRows, nColumns, i + 1)
        plt.title('Filter ' + str(i))
        plt.xticks(np.arange(0, xlen, interval), ['A', 'C', 'G', 'T'])
        plt.imshow(units[0, :, :, i], interpolation="nearest", cmap=plt.cm.bwr)
    cax = plt.axes([0.92, 0.4, 0.01, 0.3])
    plt.colorbar(cax=cax)
    plot.savefig(ofn, dpi=DPI, transparent=True, bbox_inches='tight')
    plt.close(plot)


def PlotFiltersFC(ofn, units, interval=10, xsize=18, ysize=4, xts=1, yts=1, lts=2):
    matplotlib, plt = _pyplot()
    matplotlib.rc('xtick', labelsize=xts)
    matplotlib.rc('ytick', labelsize=yts)
    matplotlib.rc('axes', titlesize=lts)
    plot = plt.figure(1, figsize=(xsize, ysize))
    cell = units.shape[1]
    plt.xticks(np.arange(0, cell, interval))
    plt.yticks(np.arange(0, 1, 1), [''])
    plt.title(str(cell) + ' units')
    plt.imshow(np.reshape(units[0, :], (-1, cell)), interpolation="nearest", cmap=plt.cm.bwr)
    cax = plt.axes([0.45, 0.05, 0.2, 0.05])
    plt.colorbar(cax=cax, orientation="horizontal")
    plot.savefig(ofn, dpi=DPI, transparent=True, bbox_inches='tight')
    plt.close(plot)


def PlotOutputArray(ofn, unitsX, unitsY, interval=1, xsize=8, ysize=2, xts=1, yts=1, lts=2):
    matplotlib, plt = _pyplot()
    matplotlib.rc('xtick', labelsize=xts)
    matplotlib.rc('ytick', labelsize=yts)
    matplotlib.rc('axes', titlesize=lts)
    plot = plt.figure(1, figsize=(xsize, ysize))
    cell = unitsX.shape[1]
    plt.subplot(2, 1, 1)
    plt.xticks(np.arange(0, cell, interval), OUTPUT_TICKS)
    plt.yticks(np.arange(0, 1, 1), [''])
    plt.title("Predicted")
    plt.imshow(np.reshape(unitsX[0, :], (-1, cell)), interpolation="nearest", cmap=plt.cm.bwr)
    plt.subplot(2, 1, 2)
    plt.xticks(np.arange(0, cell, interval), OUTPUT_TICKS)
    plt.yticks(np.arange(0, 1, 1), [''])
    plt.title("Truth")
    plt.imshow(np.reshape(unitsY[0, :], (-1, cell)), interpolation="nearest", cmap=plt.cm.bwr)
    plt.colorbar(orientation="horizontal", pad=0.5)
    plot.savefig(ofn, dpi=DPI, transparent=True, bbox_inches='tight')
    plt.close(plot)


def PlotTensor(ofn, XArray):
    _matplotlib, plt = _pyplot()
    plot = plt.figure(figsize=(15, 8))
    for k in range(4):
        plt.subplot(4, 1, k + 1); plt.xticks(np.arange(0, 33, 1)); plt.yticks(np.arange(0, 4, 1), ['A', 'C', 'G', 'T'])
        if k == 0:
            plt.imshow(XArray[0, :, :, 0].transpose(), vmin=0, vmax=50, interpolation="nearest", cmap=plt.cm.hot)
        else:
            plt.imshow(XArray[0, :, :, k].transpose(), vmin=-50, vmax=50, interpolation="nearest", cmap=plt.cm.bwr)
        plt.colorbar()
    plot.savefig(ofn, dpi=DPI, transparent=True, bbox_inches='tight')
    plt.close(plot)


def CreatePNGs(args, m, utils, total, XC, YC, posC, block=BLOCK):
    """getTensorAndLayerPNG.py:111-146, the network asked once per block of candidates instead of nine times per candidate"""
    for lo in range(0, total, block):
        XBlock, num, _ = utils.DecompressArray(XC, lo, block, total)
        YBlock, _, _ = utils.DecompressArray(YC, lo, block, total)
        posBlock, _, _ = utils.DecompressArray(posC, lo, block, total)
        got = m.layers(XBlock, LAYERS)
        for i in range(num):
            pos = posBlock[i]
            if isinstance(pos, bytes):
                pos = pos.decode()
            varName = "-".join(str(pos).split(":"))
            sys.stderr.write("Plotting %s...\n" % (varName))
            if not os.path.exists(varName):
                os.makedirs(varName)
            PlotTensor(varName + "/tensor.png", np.asarray(XBlock[i:i + 1]))
            PlotFiltersConv(varName + "/conv1.png", got["conv1"][i:i + 1], 1, 8, 9, 5, 5, 8)
            PlotFiltersConv(varName + "/conv2.png", got["conv2"][i:i + 1], 1, 8, 18, 6, 6, 9)
            PlotFiltersConv(varName + "/conv3.png", got["conv3"][i:i + 1], 1, 8, 24, 7, 7, 10)
            PlotFiltersFC(varName + "/fc4.png", got["fc4"][i:i + 1], 10, 16, 1, 9, 9, 10)
            PlotFiltersFC(varName + "/fc5.png", got["fc5"][i:i + 1], 10, 4, 1, 4, 4, 5)
            unitsX = np.concatenate([got[k][i:i + 1] for k in LAYERS[5:]], axis=1)
            unitsY = np.reshape(np.asarray(YBlock[i]), (1, -1))
            PlotOutputArray(varName + "/output.png", unitsX, unitsY, 1, 4, 2, 4, 4, 5)


_CLI = (
    ("--tensor_fn", str, "vartensors", "Tensor input"),
    ("--var_fn", str, None, "Truth variants input"),
    ("--chkpnt_fn", str, None, "Input a checkpoint for testing or continue training"),
)
_SWITCHES = (("--slim", False, "Train using the slim version of Clairvoyante, default: False"),)


def ParseArgs():
    from .train import build_parser
    parser = build_parser("Visualize tensors and hidden layers in PNG", _CLI, _SWITCHES)
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    return args


def main():
    args = ParseArgs()
    _pyplot()                       # a missing matplotlib ends the run before the model is built
    m, utils, total, XC, YC, posC = Prepare(args)
    CreatePNGs(args, m, utils, total, XC, YC, posC)


if __name__ == "__main__":
    main()
