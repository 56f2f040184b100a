"""Embeddings of the four heads for the TensorBoard projector: command line and outputs of
/root/reference/clairvoyante/getEmbedding.py (prepare_data :17-42, get_labels :59-82, visualize_embedding :85-140).

    python -m clairvoyante_amd.getEmbedding --bin_fn TENSORS.bin --chkpnt_fn MODEL --olog_dir OLOG [--count N] [--slim]

For the first --count candidates of the set it writes into OLOG
  * the metadata files BaseChange.tsv / Zygosity.tsv / VarType.tsv / IndelLength.tsv by get_labels' rules, where
    write_metadata (:44-53) puts them: OLOG/<basename of OLOG>/NAME.tsv;
  * model.ckpt-1 (.index, .data-00000-of-00001) and the `checkpoint` state file: a TensorFlow V2 bundle with the
    float32 variables BaseChange [count,4], Zygosity [count,2], VarType [count,4], IndelLength [count,6] -- the base
    head's sigmoid and the logits selu(FC) + 1e-10 of the other three (embedding1..4, v3.py:154-158; model.embeddings);
  * projector_config.pbtxt in the text form projector.visualize_embeddings writes.
No event file with the graph is written (the reference's tf.summary.FileWriter(olog_dir, sess.graph)): there is no
TensorFlow here, and the projector reads the three items above.
"""
import os
import sys

if __package__ in (None, ""):      # run as `python <dir>/getEmbedding.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
import numpy as np

from . import param

VARIABLES = ("BaseChange", "Zygosity", "VarType", "IndelLength")


def prepare_data(args):
    """getEmbedding.py:17-42"""
    from . import utils_v2 as utils
    if args.slim:
        from . import clairvoyante_v3_slim as cv
    else:
        from . import clairvoyante_v3 as cv
    utils.SetupEnv()
    m = cv.Clairvoyante()
    m.init()
    m.restoreParameters(args.chkpnt_fn)
    if args.bin_fn is not None:
        total, XC, YC, posC = utils.LoadBin(args.bin_fn)
    else:
        total, XC, YC, posC = utils.GetTrainingArray(args.tensor_fn, args.var_fn, args.bed_fn)
    return m, utils, total, XC, YC, posC


def metadata_path(olog_dir, fn):
    """where write_metadata (:44-53) puts the file the config names as `fn`: one directory level further down"""
    return os.path.dirname(fn) + "/" + os.path.basename(os.path.normpath(olog_dir)) + "/" + os.path.basename(fn)


def write_metadata(olog_dir, fn, labels):
    path = metadata_path(olog_dir, fn)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for label in labels:
            f.write("{}\n".format(label))


def get_labels(YBatch):
    """getEmbedding.py:59-82: the base head's four values per row under a header line; for the other heads one word per
    column that equals exactly 1 (a het-indel row of 0.5 / 0.5 gives no zygosity line)."""
    dict2 = {0: 'HET', 1: 'HOM'}
    dict3 = {0: 'REF', 1: 'SNP', 2: 'INS', 3: 'DEL'}
    dict4 = {0: '0', 1: '1', 2: '2', 3: '3', 4: '4', 5: '>4'}
    labels1 = ["A\tC\tG\tT"]
    for l in YBatch[:, 0:4]:
        labels1.append("%f\t%f\t%f\t%f" % (l[0], l[1], l[2], l[3]))
    labels2 = [dict2[i] for l in YBatch[:, 4:6] for i in range(2) if l[i] == 1]
    labels3 = [dict3[i] for l in YBatch[:, 6:10] for i in range(4) if l[i] == 1]
    labels4 = [dict4[i] for l in YBatch[:, 10:16] for i in range(6) if l[i] == 1]
    return labels1, labels2, labels3, labels4


def _text_string(s):
    """a string field as protobuf's text format prints it (C escapes, bytes beyond ASCII in octal)"""
    out = []
    for b in s.encode("utf-8"):
        c = chr(b)
        if c == "\n": out.append("\\n")
        elif c == "\r": out.append("\\r")
        elif c == "\t": out.append("\\t")
        elif c in "\"'\\": out.append("\\" + c)
        elif 32 <= b < 127: out.append(c)
        else: out.append("\\%03o" % b)
    return '"%s"' % "".join(out)


def projector_config(olog_dir):
    """ProjectorConfig with the four embeddings, text format (projector.visualize_embeddings -> projector_config.pbtxt)"""
    return "".join("embeddings {\n  tensor_name: %s\n  metadata_path: %s\n}\n"
                   % (_text_string(name + ":0"), _text_string(os.path.join(olog_dir, name + ".tsv"))) for name in VARIABLES)


def visualize_embedding(args, m, utils, total, XC, YC, olog_dir, embed_count):
    """getEmbedding.py:85-140"""
    from . import tf_checkpoint
    XBatch, _n, _e = utils.DecompressArray(XC, 0, embed_count, total)
    YBatch, _n, _e = utils.DecompressArray(YC, 0, embed_count, total)
    embeddings = m.embeddings(XBatch)
    labels = get_labels(np.asarray(YBatch))
    for name, lab in zip(VARIABLES, labels):
        write_metadata(olog_dir, os.path.join(olog_dir, name + ".tsv"), lab)
    os.makedirs(olog_dir, exist_ok=True)
    base = "model.ckpt-1"                                  # saver.save(sess, olog_dir/model.ckpt, 1)
    tf_checkpoint.write_bundle(os.path.join(olog_dir, base),
                               {name: np.ascontiguousarray(e, dtype=np.float32) for name, e in zip(VARIABLES, embeddings)})
    with open(os.path.join(olog_dir, "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (base, base))
    with open(os.path.join(olog_dir, "projector_config.pbtxt"), "w") as f:
        f.write(projector_config(olog_dir))


_CLI = (
    ("--bin_fn", str, None, "Binary tensor input generated by tensor2Bin.py, tensor_fn, var_fn and bed_fn will be ignored"),
    ("--tensor_fn", str, "vartensors", "Tensor input"),
    ("--var_fn", str, "truthvars", "Truth variants list input"),
    ("--bed_fn", str, None, "High confident genome regions input in the BED format"),
    ("--chkpnt_fn", str, None, "Input a checkpoint for testing or continue training"),
    ("--olog_dir", str, None, "Directory for tensorboard log outputs"),
    ("--count", int, 10000, "Number of variants to be visualized, default: 10000"),
)
_SWITCHES = (("--slim", False, "Train using the slim version of Clairvoyante, default: False"),)


def get_arguements():
    from .train import build_parser
    parser = build_parser("Get Embedding for TensorBoard Visualization", _CLI, _SWITCHES)
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    if args.olog_dir is None:
        sys.exit("getEmbedding: --olog_dir is required (the directory the projector files go to)")
    return args


def main():
    args = get_arguements()
    m, utils, total, XC, YC, _posC = prepare_data(args)
    visualize_embedding(args, m, utils, total, XC, YC, args.olog_dir, args.count)


if __name__ == "__main__":
    main()
