"""Write tests/golden/g15_fit.npz: the two schedule functions of the 3DGS reference implementation that fit.py restates, as numbers.

    python tools/gen_fit_golden.py <path of the reference checkout> [--out tests/golden/g15_fit.npz]

The reference's utils.general_utils is imported from the given path and its own functions are run:
  - the exponential rate function, called as its scene/gaussian_model.py calls it (lr_init and lr_final times spatial_lr_scale,
    lr_delay_mult 0.01, max_steps 30000), at iterations 1, 2, 100, 1000, 15000, 30000 and 40000, for the default arguments
    (spatial_lr_scale 1) and for spatial_lr_scale = 3.7;
  - inverse_sigmoid(min(sigmoid(x), 0.01)) in fp64 for 64 logits spanning -12 to 12: what its reset_opacity leaves.
Data only.  Prints max |fit.py's restatement - reference| for both."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = (1, 2, 100, 1000, 15000, 30000, 40000)
SCALES = (1.0, 3.7)
INIT, FINAL, DELAY_MULT, MAX_STEPS, CEILING = 1.6e-4, 1.6e-6, 0.01, 30000, 0.01


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g15_fit.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import general_utils                                                # the reference's own module

    rates = np.empty((len(SCALES), len(ITERATIONS)), np.float64)
    for i, scale in enumerate(SCALES):
        fn = general_utils.get_expon_lr_func(lr_init=INIT * scale, lr_final=FINAL * scale, lr_delay_mult=DELAY_MULT, max_steps=MAX_STEPS)
        rates[i] = [fn(it) for it in ITERATIONS]
    logits = np.linspace(-12.0, 12.0, 64)
    x = torch.from_numpy(logits)
    reset = general_utils.inverse_sigmoid(torch.min(torch.sigmoid(x), torch.ones_like(x) * CEILING)).numpy()
    np.savez_compressed(args.out, iterations=np.asarray(ITERATIONS, np.int64), spatial_lr_scales=np.asarray(SCALES, np.float64), position_lr=rates,
                        position_lr_args=np.asarray([INIT, FINAL, DELAY_MULT, MAX_STEPS], np.float64), logits=logits, reset_ceiling=np.float64(CEILING),
                        reset=reset)
    fit = importlib.import_module("6dgs_amd.fit")
    mine = np.array([[fit.position_lr(it, INIT, FINAL, MAX_STEPS, scale, DELAY_MULT) for it in ITERATIONS] for scale in SCALES])
    print(f"position rate: max relative |restatement - reference| {float(np.abs(mine / rates - 1.0).max()):.3e}")
    o = np.minimum(1.0 / (1.0 + np.exp(-logits)), CEILING)
    print(f"reset: max |restatement - reference| {float(np.abs(np.log(o / (1.0 - o)) - reset).max()):.3e}")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
