#!/usr/bin/env python3
"""Generates tests/golden/embedding_labels.json: the metadata lines the reference's own get_labels
(getEmbedding.py:59-82) gives for 40 label rows (run in the build container only; the reference never travels,
and no test runs this file).

    python tests/golden/make_golden_embedding_labels.py

The reference file imports TensorFlow at module level, so it is not imported: it is copied to a temp dir OUTSIDE the
repo, passed through 2to3 (as make_golden_ref.py does), and the one function is lifted out of the copy and executed
(it needs nothing but xrange).  Only the inputs and the reference's outputs are stored (data, not source).
"""
import ast
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/clairvoyante"


def reference_get_labels():
    tmp = tempfile.mkdtemp(prefix="cv_ref23_")
    try:
        fn = os.path.join(tmp, "getEmbedding.py")
        shutil.copy(os.path.join(REF, "getEmbedding.py"), fn)
        subprocess.call([sys.executable, "-m", "lib2to3", "-nw", fn], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        src = open(fn).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    node = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_labels"][0]
    ns = {"xrange": range}            # (only read where 2to3 is not there to rewrite it)
    exec(compile(ast.Module(body=[node], type_ignores=[]), "getEmbedding.py", "exec"), ns)
    return ns["get_labels"]


def label_rows():
    """40 rows of GetTrainingArray's kind (float64 [n,16], utils_v2.py:62-186): homozygous and heterozygous SNPs (base
    columns 1 or 0.5 / 0.5), het indels whose ZYGOSITY columns are 0.5 / 0.5, every variant type and indel length."""
    y = np.zeros((40, 16), dtype=np.float64)
    for i in range(40):
        if i % 5 == 3:
            y[i, i % 4] = 0.5; y[i, (i + 1 + i // 4) % 4] += 0.5        # two bases (or one, twice)
        else:
            y[i, i % 4] = 1.0
        if i % 7 == 2:
            y[i, 4] = 0.5; y[i, 5] = 0.5                                # no zygosity line for this row
        else:
            y[i, 4 + (i // 2) % 2] = 1.0
        y[i, 6 + (i // 3) % 4] = 1.0
        y[i, 10 + i % 6] = 1.0
    assert (y != 0).any(axis=0).all()
    return y


def main():
    y = label_rows()
    l1, l2, l3, l4 = reference_get_labels()(y)
    with open(os.path.join(HERE, "embedding_labels.json"), "w") as f:
        json.dump({"y": y.tolist(), "BaseChange": l1, "Zygosity": l2, "VarType": l3, "IndelLength": l4}, f, indent=0)
        f.write("\n")
    print("embedding_labels.json: %d rows -> %d / %d / %d / %d lines" % (len(y), len(l1), len(l2), len(l3), len(l4)))


if __name__ == "__main__":
    main()
