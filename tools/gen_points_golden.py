"""Write tests/golden/g16_points.npz: what the 3DGS reference implementation computes and reads when it starts a scene from points.

    python tools/gen_points_golden.py <path of the reference checkout> [--out tests/golden/g16_points.npz]

The reference's own modules are imported from the given path and run on the CPU:
  * utils.sh_utils.RGB2SH on 300 fp32 colours in [0, 1] and utils.general_utils.inverse_sigmoid on 0.1 (and on a few more
    probabilities), both in torch fp32 as GaussianModel.create_from_pcd calls them;
  * scene.colmap_utils.read_points3D_binary / read_points3D_text on a points3D.bin and a points3D.txt of 50 points that THIS tool
    writes (COLMAP's layout, tracks of varying length): the files' bytes are stored with what the two readers return for them.
Data only: no text of the reference.  The nearest-neighbour distances (distCUDA2) are not part of this golden: that extension does not
run on a CPU, and include/sixdgs.h defines the result to the bit instead."""
import argparse
import importlib.util
import os
import struct
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_points3d(rng, n):
    """-> (bytes of points3D.bin, text of points3D.txt) for the same n points."""
    xyz = rng.normal(0.0, 3.0, (n, 3))
    rgb = rng.integers(0, 256, (n, 3))
    err = rng.random(n) * 2.0
    ids = np.sort(rng.choice(10 * n, n, replace=False)) + 1
    blob = [struct.pack("<Q", n)]
    lines = ["# 3D point list with one line of data per point:", "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)",
             f"# Number of points: {n}", ""]
    for i in range(n):
        track = rng.integers(1, 500, (int(rng.integers(0, 6)), 2))
        blob.append(struct.pack("<QdddBBBd", int(ids[i]), *xyz[i], *[int(c) for c in rgb[i]], err[i]))
        blob.append(struct.pack("<Q", track.shape[0]) + b"".join(struct.pack("<ii", int(a), int(b)) for a, b in track))
        lines.append(" ".join([str(int(ids[i]))] + [repr(float(v)) for v in xyz[i]] + [str(int(c)) for c in rgb[i]] + [repr(float(err[i]))]
                              + [str(int(v)) for v in track.reshape(-1)]))
    return b"".join(blob), "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g16_points.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import general_utils, sh_utils                                     # the reference's own modules
    # scene/colmap_utils.py by its file: importing the `scene` package would pull in the trainer's CUDA extensions
    spec = importlib.util.spec_from_file_location("ref_colmap_utils", os.path.join(os.path.abspath(args.reference), "scene", "colmap_utils.py"))
    colmap_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(colmap_utils)

    rng = np.random.default_rng(16)
    rgb = rng.random((300, 3)).astype(np.float32)
    rgb[0], rgb[1], rgb[2] = 0.0, 1.0, 0.5
    sh = sh_utils.RGB2SH(torch.tensor(rgb).float()).numpy()
    prob = np.array([0.1, 0.005, 0.01, 0.5, 0.9], np.float32)
    logit = general_utils.inverse_sigmoid(torch.tensor(prob)).numpy()
    logit_init = general_utils.inverse_sigmoid(0.1 * torch.ones((7, 1), dtype=torch.float)).numpy()

    bin_bytes, txt = write_points3d(rng, 50)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "points3D.bin"), "wb") as f:
            f.write(bin_bytes)
        with open(os.path.join(d, "points3D.txt"), "w") as f:
            f.write(txt)
        b_xyz, b_rgb, b_err = colmap_utils.read_points3D_binary(os.path.join(d, "points3D.bin"))
        t_xyz, t_rgb, t_err = colmap_utils.read_points3D_text(os.path.join(d, "points3D.txt"))
    np.savez_compressed(args.out, rgb=rgb, sh=sh, prob=prob, logit=logit, logit_init=logit_init,
                        points3d_bin=np.frombuffer(bin_bytes, np.uint8), points3d_txt=np.frombuffer(txt.encode(), np.uint8),
                        bin_xyz=b_xyz, bin_rgb=b_rgb, bin_err=b_err, txt_xyz=t_xyz, txt_rgb=t_rgb, txt_err=t_err)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes; bin/txt readers agree to {float(np.abs(b_xyz - t_xyz).max()):.1e}")


if __name__ == "__main__":
    main()
