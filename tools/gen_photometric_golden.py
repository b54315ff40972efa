"""Write tests/golden/g14_photometric.npz: four small image pairs with the loss of the 3DGS reference implementation on them.

    python tools/gen_photometric_golden.py <path of the reference checkout> [--out tests/golden/g14_photometric.npz]

The reference's utils.loss_utils is imported from the given path and run in fp64 on each pair: l1_loss, ssim (11 x 11 window,
sigma 1.5), the combined (1 - 0.2) l1 + 0.2 (1 - ssim) of its train.py, and its autograd gradient of that by the first image.  The
pairs: random 5 x 7, 16 x 16 and 33 x 17, and a 24 x 40 one whose target is the image shifted by (2, 3); 3 channels.  Data only.
Prints max |fp64 restatement - reference| per stored quantity (tests/photometric_reference.py): the golden tests' bound is 8 x that.
The two differ by design in one place: the reference rounds its window to fp32 AFTER normalising in fp32 and forms the 11 x 11 outer
product in fp32; the definition takes the fp32 roundings of the fp64-normalised taps, separably."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import photometric_reference as PR  # noqa: E402

LAMBDA = 0.2


def pairs():
    rng = np.random.default_rng(14)
    out = {}
    for name, (h, w) in (("r5x7", (5, 7)), ("r16x16", (16, 16)), ("r33x17", (33, 17))):
        out[name] = (rng.random((h, w, 3), dtype=np.float32), rng.random((h, w, 3), dtype=np.float32))
    big = rng.random((24 + 2, 40 + 3, 3), dtype=np.float32)
    out["shift24x40"] = (np.ascontiguousarray(big[2:, 3:]), np.ascontiguousarray(big[:24, :40]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g14_photometric.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import loss_utils                                                   # the reference's own module

    store, worst = {"names": np.array(list(pairs()))}, {}
    for name, (image, target) in pairs().items():
        a = torch.from_numpy(image).double().permute(2, 0, 1).contiguous().requires_grad_(True)        # the reference's [3,H,W]
        b = torch.from_numpy(target).double().permute(2, 0, 1).contiguous()
        l1, ssim = loss_utils.l1_loss(a, b), loss_utils.ssim(a, b)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ssim)
        loss.backward()
        ref = {"l1": float(l1), "ssim": float(ssim), "loss": float(loss), "grad": a.grad.permute(1, 2, 0).contiguous().numpy()}
        store.update({f"{name}_image": image, f"{name}_target": target, **{f"{name}_{k}": np.asarray(v, np.float64) for k, v in ref.items()}})
        # lambda as the double 0.2 here; the C function takes it as a float, the tests allow for that rounding (3e-9 relative)
        mine = PR.evaluate(image[None], target[None], LAMBDA, np.float64)
        got = {"l1": mine["parts"][0, 0], "ssim": mine["parts"][0, 1], "loss": mine["loss"][0], "grad": mine["grad"][0]}
        for k in ref:
            err, scale = float(np.abs(got[k] - ref[k]).max()), float(np.abs(ref[k]).max())
            worst[k] = max(worst.get(k, 0.0), err / scale)
            print(f"{name:12s} {k:5s}: max |fp64 restatement - reference| {err:.3e} ({err / scale:.2e} of the scale {scale:.3e})")
    for k, v in worst.items():
        print(f"worst {k}: {v:.2e} of the scale")
    np.savez_compressed(args.out, **store)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
