"""Write tests/golden/g17_metrics.npz: four small image pairs with the evaluation numbers of the 3DGS reference implementation on them.

    python tools/gen_metrics_golden.py <path of the reference checkout> [--out tests/golden/g17_metrics.npz]

The reference's utils.loss_utils and utils.image_utils are imported from the given path and run in fp64 on each pair, once after
training_report's clamp to [0, 1] ("clamp") and once after the 8-bit rule of a saved PNG ("u8": torchvision's save_image arithmetic,
mul(255).add_(0.5).clamp_(0, 255).to(uint8), the bytes passed through a real in-memory PNG with PIL -- which must give them back
unchanged -- and to_tensor's division by 255 in fp32).  Stored per pair and mode: l1_loss, ssim on the [3,H,W] and on the [1,3,H,W]
form, and psnr on the [1,3,H,W] form (metrics.py's: one value) and on the [3,H,W] form (train.py's: the mean of three).  The pairs
are tools/gen_photometric_golden.py's sizes -- 5 x 7, 16 x 16, 33 x 17, 24 x 40 -- with values from [-0.25, 1.25].  Data only.
Prints max |fp64 restatement - reference| per quantity (tests/metrics_reference.py): the golden tests' bound is 8 x that."""
import argparse
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_reference as MR  # noqa: E402

MODES = ("clamp", "u8")
QUANTITIES = ("l1", "ssim", "ssim4", "psnr", "psnr_channels")


def pairs():
    rng = np.random.default_rng(17)
    draw = lambda h, w: (rng.random((h, w, 3), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)      # noqa: E731
    out = {name: (draw(h, w), draw(h, w)) for name, (h, w) in (("r5x7", (5, 7)), ("r16x16", (16, 16)), ("r33x17", (33, 17)))}
    big = draw(24 + 2, 40 + 3)
    out["shift24x40"] = (np.ascontiguousarray(big[2:, 3:]), np.ascontiguousarray(big[:24, :40]))
    return out


def through_png(x):
    """fp32 [H,W,3] -> (the bytes save_image writes, read back from a real PNG; to_tensor's fp32 values of them)."""
    u = torch.from_numpy(x).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    buf = io.BytesIO()
    Image.fromarray(u).save(buf, format="PNG")
    back = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    assert back.dtype == np.uint8 and np.array_equal(back, u), "the PNG round trip changed the bytes"
    return back, torch.from_numpy(back).float().div(255).numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g17_metrics.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import image_utils, loss_utils                                      # the reference's own modules

    store, worst = {"names": np.array(list(pairs()))}, {}
    for name, (image, target) in pairs().items():
        store.update({f"{name}_image": image, f"{name}_target": target})
        for mode in MODES:
            if mode == "clamp":
                a32, b32 = torch.clamp(torch.from_numpy(image), 0.0, 1.0).numpy(), torch.clamp(torch.from_numpy(target), 0.0, 1.0).numpy()
            else:
                (ua, a32), (ub, b32) = through_png(image), through_png(target)
                store.update({f"{name}_image_u8": ua, f"{name}_target_u8": ub})
            a = torch.from_numpy(a32).double().permute(2, 0, 1).contiguous()          # the reference's [3,H,W]
            b = torch.from_numpy(b32).double().permute(2, 0, 1).contiguous()
            ref = {"l1": float(loss_utils.l1_loss(a, b)), "ssim": float(loss_utils.ssim(a, b)), "ssim4": float(loss_utils.ssim(a[None], b[None])),
                   "psnr": float(image_utils.psnr(a[None], b[None]).reshape(-1)[0]), "psnr_channels": float(image_utils.psnr(a, b).mean())}
            store.update({f"{name}_{mode}_{k}": np.asarray(v, np.float64) for k, v in ref.items()})
            mine = MR.evaluate(image[None], target[None], mode == "u8", np.float64)
            got = {"l1": mine["l1"][0], "ssim": mine["ssim"][0], "ssim4": mine["ssim"][0],
                   "psnr": 10.0 * np.log10(1.0 / mine["mse"][0]), "psnr_channels": (10.0 * np.log10(1.0 / mine["mse_c"][0])).mean()}
            for k in QUANTITIES:
                err, scale = abs(float(got[k]) - ref[k]), abs(ref[k])
                worst[k] = max(worst.get(k, 0.0), err / scale)
                print(f"{name:12s} {mode:5s} {k:13s}: |fp64 restatement - reference| {err:.3e} ({err / scale:.2e} of the scale {scale:.3e})")
    for k, v in worst.items():
        print(f"worst {k}: {v:.2e} of the scale")
    np.savez_compressed(args.out, **store)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
