"""Generate the lin / lin+ model golden logits by running the REFERENCE on CPU.

Build container only (needs the reference checkout, read-only; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lin.py

Writes models_lin.npz (data only, no reference source): QAT-mode eval logits of ResNet20 lin 4-bit
and MobileNetV2 lin+ 4-bit at 32x32 on gen_golden.py's seeded input (x/cifar8 of models.npz) with
fill.seeded_fill_(seed=7) weights -- the same seeds as gen_golden.py, which stays as it is.
The logits are checked to be finite here (a constant input channel would make lin NaN).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
from fill import seeded_fill_  # noqa: E402

SPECS = [("resnet20", "lin", 4), ("mobilenet", "lin+", 4)]


def main():
    sys.path.insert(0, REF)
    from models.model import get_model
    from utils.quantizers import quantizer_dict

    torch.manual_seed(0)
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    out = {"x/cifar8": x.numpy()}
    for mt, q, bits in SPECS:
        m = get_model(mt, 10, quantizer_dict[q], bits, (32, 32))
        seeded_fill_(m, seed=7)
        m.eval()
        with torch.no_grad():
            logits = m(x).numpy()
        assert np.isfinite(logits).all(), (mt, q, bits)
        out["logits/%s/%s/%d" % (mt, q, bits)] = logits
    path = os.path.join(HERE, "models_lin.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    print("models_lin.npz:", sorted(out), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
