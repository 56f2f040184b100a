"""Float64 formulation of a training step with alpha-dropout on fc4 AND fc5 (clairvoyante_v3.py:117-151, selu.py:34-69),
built from tests/torch_ref.py's layers.  The oracle (oracle/cv_oracle.c) has no fc5 mask, so this is the reference of
tests/test_dropout5*.py.  Masks are KEEP masks (1 kept, 0 dropped): the device exports a*keep (cv_get_activation 6 / 8),
keep = mask != 0."""
import numpy as np
import torch

import torch_ref

ALPHA_P = -1.7580993408473766


def alpha_dropout(h, keep, rate):
    """selu.py:53-62 with the keep mask given: a*(h*keep + alpha'*(1-keep)) + b"""
    q = 1.0 - rate
    a = (1.0 / (q * ((1 - q) * ALPHA_P * ALPHA_P + 1.0))) ** 0.5
    b = -a * ((1 - q) * ALPHA_P)
    return a * (h * keep + ALPHA_P * (1 - keep)) + b


def heads_tail(params, d4, y, lam=0.0, mask5=None, rate5=0.0):
    """fc5 (+ its dropout) and the four heads on the fc4 output d4 (after fc4's dropout): losses (sums over the batch,
    v3.py:140-151) and the intermediates.  params: float64 tensors (may require grad)."""
    p = params
    fc5 = torch_ref.selu(d4 @ p["fc5/kernel"] + p["fc5/bias"])
    d5 = fc5
    if mask5 is not None:
        d5 = alpha_dropout(fc5, torch.as_tensor(mask5, dtype=torch.float64), rate5)
    base = torch.sigmoid(d4 @ p["YBaseChangeSigmoid/kernel"] + p["YBaseChangeSigmoid/bias"])
    lz = torch_ref.selu(d5 @ p["YZygosityFC/kernel"] + p["YZygosityFC/bias"]) + 1e-10
    lt = torch_ref.selu(d5 @ p["YVarTypeFC/kernel"] + p["YVarTypeFC/bias"]) + 1e-10
    ll = torch_ref.selu(d5 @ p["YIndelLengthFC/kernel"] + p["YIndelLengthFC/bias"]) + 1e-10
    y = torch.as_tensor(y, dtype=torch.float64)
    l1 = ((base - y[:, 0:4]) ** 2).sum()
    l2 = (-y[:, 4:6] * torch.log_softmax(lz, 1)).sum()
    l3 = (-y[:, 6:10] * torch.log_softmax(lt, 1)).sum()
    l4 = (-y[:, 10:16] * torch.log_softmax(ll, 1)).sum()
    reg = sum((v ** 2).sum() / 2 for k, v in p.items() if "bias" not in k)
    return (l1, l2, l3, l4, lam * reg), {"fc5": fc5, "d5": d5}


def loss_grad(arch, params, x, y, lam, mask4=None, rate4=0.0, mask5=None, rate5=0.0, want_pre=False):
    """-> dict: loss, parts (loss1..4, lossL2), grads {name: array} (with the lambda term), d4, fc5, d5 (arrays) and,
    with want_pre, the per-candidate pre-activation gradients of conv1..conv3 ([n, h, 4, c], data terms only)."""
    tp = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    r = torch_ref.forward(arch, tp, x, torch.float64, mask4, rate4, retain_pre=want_pre)
    parts, inter = heads_tail(tp, r["d4"], y, lam, mask5, rate5)
    total = sum(parts)
    total.backward()
    out = {"loss": float(total.detach()), "parts": [float(v.detach()) for v in parts],
           "grads": {k: v.grad.numpy() for k, v in tp.items()},
           "d4": r["d4"].detach().numpy(), "fc5": inter["fc5"].detach().numpy(), "d5": inter["d5"].detach().numpy()}
    if want_pre:
        out["pre"] = [r["pre%d_t" % (l + 1)].grad.permute(0, 2, 3, 1).numpy() for l in range(3)]
    return out
