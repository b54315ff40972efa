"""fp64 restatement of the image sixdgs_splat_views defines (include/sixdgs.h), in plain numpy, written from that text:

  1. p = W xyz + t per view ([W | t] = w2c = [R^T | T]); a Gaussian is skipped unless p.z > near_z
  2. u = fx p.x / p.z + cx, v = fy p.y / p.z + cy, r = max(extent * max(exp(log_scale)) * fx / p.z, 0.7072)
  3. it covers pixel (x, y) when (x + 0.5 - u)^2 + (y + 0.5 - v)^2 <= r^2, at depth p.z
  4. winner = the covering Gaussian of smallest p.z, equal p.z -> smaller index
  5. colour = round(255 min(SH colour towards the camera, 1)); background elsewhere

Inputs are the fp32 numbers the kernel gets (scene arrays, camera rows), widened to fp64; everything after that is fp64.

A pixel is UNDECIDABLE when fp32 rounding may legitimately change its winner:
  (a) the two nearest covering depths differ by less than DEPTH_TIE relative, or
  (b) some Gaussian not behind the winner has |d^2 - r^2| < edge_tol r^2 there (a disc edge passes through the pixel centre).
edge_tol = 1e-4 comes from the projection's fp32 error at <= 160-pixel images (about 1e-5 px in u, v against r >= 0.7); it grows with
the image size and is not valid for 800-pixel images.
"""
import math

import numpy as np

DEPTH_TIE = 1e-6
EDGE_TOL = 1e-4
MAX_UNDECIDABLE_SHARE = 1e-3      # of a case's pixels

# the three cases of the winner test: (Gaussians, scene seed, views, camera seed, width, height); FoV 0.8, extent 1, near_z 0.05
WINNER_CASES = ((2000, 3, 4, 4, 128, 128), (2000, 5, 4, 6, 160, 120), (5000, 7, 2, 8, 128, 128))


def camera_rows(cams):
    """[V,16] fp32 -- w2c rows 0..2 ([R^T | T]), fx, fy, cx, cy: what the kernel is given."""
    out = np.empty((len(cams), 16), np.float32)
    for i, c in enumerate(cams):
        w2c = np.concatenate([np.asarray(c["R"], np.float64).T, np.asarray(c["T"], np.float64).reshape(3, 1)], axis=1)
        out[i, :12] = w2c.reshape(-1)
        out[i, 12] = c["width"] / (2 * math.tan(c["FovX"] / 2))
        out[i, 13] = c["height"] / (2 * math.tan(c["FovY"] / 2))
        out[i, 14], out[i, 15] = c["width"] / 2, c["height"] / 2
    return out


def camera_centre(row):
    m = np.asarray(row, np.float64)[:12].reshape(3, 4)
    return -m[:, :3].T @ m[:, 3]


def project(xyz, log_scale, row, extent, near_z):
    """-> z, visible, u, v, r (fp64 [n]) for one view."""
    row = np.asarray(row, np.float64)
    m = row[:12].reshape(3, 4)
    fx, fy, cx, cy = row[12:]
    p = np.asarray(xyz, np.float64) @ m[:, :3].T + m[:, 3]
    z = p[:, 2]
    vis = z > near_z
    zs = np.where(vis, z, 1.0)
    u, v = fx * p[:, 0] / zs + cx, fy * p[:, 1] / zs + cy
    r = np.maximum(extent * np.exp(np.asarray(log_scale, np.float64)).max(-1) * fx / zs, 0.7072)
    return z, vis, u, v, r


def reference_view(xyz, log_scale, row, width, height, extent=1.0, near_z=0.05, edge_tol=EDGE_TOL, chunk=256):
    """One view -> (winner int64 [H,W] (-1: none), undecidable bool [H,W])."""
    z, vis, u, v, r = project(xyz, log_scale, row, extent, near_z)
    # Gaussians whose disc (with room for the edge band) reaches the frame; the others cover nothing
    reach = vis & (u + 1.01 * r + 1 > 0) & (u - 1.01 * r - 1 < width) & (v + 1.01 * r + 1 > 0) & (v - 1.01 * r - 1 < height)
    ids = np.nonzero(reach)[0]
    px, py = np.arange(width) + 0.5, np.arange(height) + 0.5
    z1 = np.full((height, width), np.inf)
    z2 = np.full((height, width), np.inf)
    zn = np.full((height, width), np.inf)
    win = np.full((height, width), -1, np.int64)
    for c0 in range(0, ids.shape[0], chunk):
        g = ids[c0:c0 + chunk]                  # ascending indices: ties keep the smaller one below
        d2 = (px[None, None, :] - u[g, None, None]) ** 2 + (py[None, :, None] - v[g, None, None]) ** 2
        r2 = (r[g] ** 2)[:, None, None]
        zg = z[g][:, None, None]
        zz = np.where(d2 <= r2, zg, np.inf)
        first = zz.argmin(axis=0)               # first occurrence of the minimum = smallest index
        c1 = np.take_along_axis(zz, first[None], axis=0)[0]
        if zz.shape[0] > 1:
            np.put_along_axis(zz, first[None], np.inf, axis=0)
            c2 = zz.min(axis=0)
        else:
            c2 = np.full_like(c1, np.inf)
        better = c1 < z1
        z2 = np.minimum(np.maximum(z1, c1), np.minimum(z2, c2))
        win = np.where(better, g[first], win)
        z1 = np.minimum(z1, c1)
        zn = np.minimum(zn, np.where(np.abs(d2 - r2) < edge_tol * r2, zg, np.inf).min(axis=0))
    with np.errstate(invalid="ignore"):       # inf - inf where nothing covers the pixel
        tie = np.isfinite(z2) & ((z2 - z1) < DEPTH_TIE * z1)
    edge = np.isfinite(zn) & (zn <= z1 * (1 + DEPTH_TIE))
    return win, tie | edge


def reference_views(scene, rows, width, height, extent=1.0, near_z=0.05, edge_tol=EDGE_TOL):
    out = [reference_view(scene["xyz"], scene["log_scale"], row, width, height, extent, near_z, edge_tol) for row in rows]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def ray_dirs_to_camera(xyz, row):
    """normalize(camera centre - xyz): the direction of a ray that leaves each Gaussian towards the camera (fp64)."""
    d = camera_centre(row)[None] - np.asarray(xyz, np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)
