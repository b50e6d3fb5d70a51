"""Generate tests/golden/focal_v1.npz by running the REAL reference's FocalLossV1 (model/PMMA/
paired_multi_model_attention_model.py:32-67, reduction='mean') on the CPU in fp64.

    python tests/golden/make_focal_golden.py

The file holds data only: the inputs (z, y: 257 rows, |z| up to 20, hard labels and a block of soft ones) and, for each
(alpha, gamma) of SETTINGS, the reference's loss and d loss / d z from its own autograd.  Nothing of the reference is copied;
it is imported at generation time, as make_golden.py does.  tests/test_cls_loss_reference_cpu.py compares the fp64 formula
of tests/cls_loss_ref.py against it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SETTINGS = ((0.25, 2), (0.5, 1), (0.75, 3))
N = 257


def main():
    import ref_harness
    ref_harness.import_reference()
    from model.PMMA.paired_multi_model_attention_model import FocalLossV1
    g = torch.Generator().manual_seed(20240611)
    z = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * 20.0
    z[0], z[1], z[2] = 20.0, -20.0, 0.125
    y = (torch.rand(N, generator=g) < 0.3).double()
    y[0], y[1] = 1.0, 0.0
    y[200:] = torch.rand(N - 200, generator=g, dtype=torch.float64)
    out = {"z": z.numpy(), "y": y.numpy(), "settings": np.array(SETTINGS, dtype=np.float64)}
    for k, (alpha, gamma) in enumerate(SETTINGS):
        zz = z.clone().requires_grad_(True)
        loss = FocalLossV1(alpha=alpha, gamma=gamma, reduction="mean")(zz, y)
        loss.backward()
        out["loss_%d" % k] = np.array(float(loss.detach()))
        out["grad_%d" % k] = zz.grad.numpy()
    path = os.path.join(HERE, "focal_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
