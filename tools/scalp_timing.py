"""Time of the scalp labelling (csrc/hgs_scalp.hip through utils/scalp.py): a generated head -- an icosphere of 5 subdivisions stretched
to an ellipsoid, 20 480 faces -- against --views views of 1000x1000 on a ring with a little height, masks set where the pixel's ray
first meets the head above z = 0.25, and --samples samples (the vertices, then face points of surface_samples).  GPU ms, each the
median of --reps launches between device events after a warm-up, buffers resident: hgs_scalp_depth (the +inf fill included) over all
views, hgs_scalp_votes over all samples.  Then label_scalp end to end from host arrays to host arrays on the device (uploads, packing,
both kernels, copies back; one run after a warm-up) and on the numpy path of the same tree, and whether the two results are equal.
There is no earlier implementation to race: the device path is reported against the numpy path.  Prints one JSON line and writes it
to profiles/scalp_timing.json (--out).
  python tools/scalp_timing.py [--views 64] [--samples 50000] [--reps 7] [--no_numpy] [--out profiles/scalp_timing.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np

from carve_timing import events, look_at

W, H, F = 1000, 1000, 1100.0
AXES = np.array([0.8, 0.9, 1.0])            # the head's half axes
RING = 4.0                                  # the cameras' distance from its centre
MIN_COS, DEPTH_TOL, MIN_VIEWS, MIN_PERCENT = 0.25, 0.02, 2, 70


def icosphere(subdivisions):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in
             ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts), np.array(faces, np.int64)


def capture(V):
    """(views, masks): a pixel is set iff the ray through its centre first meets the ellipsoid at z > 0.25."""
    from utils.carve import View
    views, masks = [], []
    xs, ys = (np.arange(W) + 0.5 - W / 2) / F, (np.arange(H) + 0.5 - H / 2) / F
    d_cam = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.ones((H, W))), axis=-1)
    for k in range(V):
        a = 2.0 * np.pi * k / V
        c = np.array([RING * np.cos(a), RING * np.sin(a), 1.0 + 0.8 * np.sin(3 * a)])
        R, t = look_at(c)
        views.append(View(R=R, t=t, fx=F, fy=F, cx=W / 2, cy=H / 2, W=W, H=H, name=f"view_{k:02d}.png"))
        d = (d_cam @ R) / AXES                                   # world directions, in the space where the head is the unit sphere
        o = c / AXES
        dd, b = (d * d).sum(-1), d @ o
        disc = b * b - dd * (o @ o - 1.0)
        s = (-b - np.sqrt(np.maximum(disc, 0.0))) / dd
        z = c[2] + s * (d[..., 2] * AXES[2])
        masks.append(np.where((disc > 0.0) & (s > 0.0) & (z > 0.25), 255, 0).astype(np.uint8))
    return views, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no_numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalp_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "scalp_timing.py measures the GPU path: it needs the GPU"
    import hgs_runtime as rt
    from utils import carve, scalp
    verts, faces = icosphere(5)
    verts = verts * AXES
    views, masks = capture(a.views)
    points, normals = scalp.surface_samples(verts, faces, 0.03)
    points, normals = np.ascontiguousarray(points[:a.samples]), np.ascontiguousarray(normals[:a.samples])
    res = {"device": torch.cuda.get_device_name(0), "faces": int(faces.shape[0]), "vertices": int(verts.shape[0]), "views": a.views,
           "view_size": [W, H], "samples": int(points.shape[0]), "reps": a.reps, "depth_bytes": 8 * W * H * a.views,
           "min_cos": MIN_COS, "depth_tol": DEPTH_TOL}
    packed = carve.pack(views, masks, None, "cuda")
    v_dev, f_dev = torch.from_numpy(verts).cuda(), torch.from_numpy(faces.astype(np.int32)).cuda()
    p_dev, n_dev = torch.from_numpy(points).cuda(), torch.from_numpy(normals).cuda()
    depth, dropped = scalp.depth_device(v_dev, f_dev, packed)
    res["dropped"] = dropped
    res["covered_pixels"] = int(torch.isfinite(depth).sum())
    drop_dev = torch.empty(1, dtype=torch.int64, device="cuda")
    L, V = rt.lib(), len(views)

    def depth_launch():
        rt.check(L.hgs_scalp_depth(rt.current_stream(), verts.shape[0], rt.ptr(v_dev), faces.shape[0], rt.ptr(f_dev), V, rt.ptr(packed.views_dev),
                                   rt.ptr(depth), rt.ptr(drop_dev)))
    d_ms = events(depth_launch, a.reps)
    vis, hits = scalp.votes_device(p_dev, n_dev, packed, depth, MIN_COS, DEPTH_TOL)
    v_ms = events(lambda: scalp.votes_device(p_dev, n_dev, packed, depth, MIN_COS, DEPTH_TOL), a.reps)
    res.update({"depth_ms": round(d_ms, 3), "depth_face_views_per_s": round(faces.shape[0] * V / d_ms * 1e3),
                "depth_fill_GB_per_s_lower_bound": round(8 * W * H * V / d_ms / 1e6, 1),
                "votes_ms": round(v_ms, 3), "votes_projections_per_s": round(points.shape[0] * V / v_ms * 1e3),
                "visible_pairs": int(vis.sum()), "hit_pairs": int(hits.sum())})
    # label_scalp, host arrays to host arrays (its samples are all of surface_samples' at this spacing)
    spacing = 0.03
    args = (verts, faces, views, masks, spacing, MIN_COS, DEPTH_TOL, MIN_VIEWS, MIN_PERCENT)
    scalp.label_scalp(*args, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = scalp.label_scalp(*args, device="cuda")
    res["label_samples"] = int(got[1].shape[0])
    res["label_kept"] = int(got[3].sum())
    res["label_device_s"] = round(time.perf_counter() - t0, 3)
    if not a.no_numpy:
        t0 = time.perf_counter()
        want = scalp.label_scalp(*args)
        res["label_numpy_s"] = round(time.perf_counter() - t0, 2)
        res["device_equals_numpy"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
