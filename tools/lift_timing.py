"""Time of the direction lift (csrc/hgs_lift.hip through utils/lift.py): --points points on an ellipsoid against --views views of
1920x1080 whose masks are its analytic silhouettes (tools/carve_timing.py's capture) and whose orientation maps are, per pixel, the
image angle of a combed tangent field (the surface tangent orthogonal to the world z axis) at the point the pixel's ray meets the
ellipsoid first; confidence 255 on the mask.  Nothing is occluded in the masks, but every point is also in frame of the far-side
views, which see the near side's hair at that pixel: the re-weighted rounds are what copes with those.  GPU ms, each the median of
--reps runs between device events after a warm-up, buffers resident: hgs_lift_moments without and with a previous direction,
hgs_lift_solve, and lift_directions' device loop (rounds + 1 of each); the upload of the planes; and the numpy path's seconds for the
same lift_directions call on the same points -- the parent of this step has no such stage, so the host path is the only baseline
there is.  Also records, as a measurement, the median angle between the lifted directions and the field at the points, after round
0 and after the last round, and that the two backends' moments are equal.  Prints one JSON line and writes it to
profiles/lift_timing.json (--out).
  python tools/lift_timing.py [--points 200000] [--views 32] [--rounds 3] [--reps 7] [--no_numpy] [--out profiles/lift_timing.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd"), os.path.dirname(os.path.abspath(__file__))]

import numpy as np

from carve_timing import AXES, F, H, W, capture, events


def field(p):
    """Unit tangents [n, 3] of the combed field at surface points p [n, 3]: normal x e_z (zero at the poles)."""
    n = p / (AXES * AXES)
    t = np.stack([n[..., 1], -n[..., 0], np.zeros_like(n[..., 0])], axis=-1)
    return t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-300)


def orientation_maps(views, masks):
    """(orients, confs): per view, the byte of the image angle of the field at the first hit of every mask pixel's ray."""
    xs, ys = (np.arange(W) + 0.5 - W / 2) / F, (np.arange(H) + 0.5 - H / 2) / F
    orients, confs = [], []
    for v, m in zip(views, masks):
        py, px = np.nonzero(m)
        d = np.stack([xs[px], ys[py], np.ones(px.size)], axis=-1) @ v.R          # world ray directions
        c = -v.R.T @ v.t
        ds, cs = d / AXES, c / AXES                              # the space where the ellipsoid is the unit sphere
        A, B, C = (ds * ds).sum(-1), (ds * cs).sum(-1), (cs * cs).sum() - 1.0
        s = (-B - np.sqrt(np.maximum(B * B - A * C, 0.0))) / A
        p = c + s[:, None] * d
        pc, tc = p @ v.R.T + v.t, field(p) @ v.R.T
        du = v.fx * (tc[:, 0] * pc[:, 2] - pc[:, 0] * tc[:, 2])
        dv = v.fy * (tc[:, 1] * pc[:, 2] - pc[:, 1] * tc[:, 2])
        o = np.zeros((H, W), np.uint8)
        o[py, px] = np.mod(np.rint(np.mod(np.arctan2(du, dv), np.pi) * 255.0 / np.pi), 256).astype(np.uint8)
        orients.append(o)
        confs.append(np.where(m != 0, 255, 0).astype(np.uint8))
    return orients, confs


def median_angle(d, truth):
    has = d.any(axis=1)
    c = np.abs((d[has] * truth[has]).sum(axis=1))
    return round(float(np.degrees(np.median(np.arccos(np.clip(c, 0.0, 1.0))))), 3), int(has.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma_deg", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no_numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "lift_timing.py measures the GPU path: it needs the GPU"
    from utils import lift
    views, masks = capture(a.views)
    orients, confs = orientation_maps(views, masks)
    rng = np.random.default_rng(0)
    u = rng.normal(size=(a.points, 3))
    u[:, 2] *= 0.8                                               # (fewer points at the poles, where the field is singular)
    pts = np.ascontiguousarray(u / np.linalg.norm(u, axis=1, keepdims=True) * AXES)
    truth = field(pts)
    s2 = lift.sin2(a.sigma_deg)
    res = {"device": torch.cuda.get_device_name(0), "points": a.points, "views": a.views, "view_size": [W, H], "rounds": a.rounds,
           "sigma_deg": a.sigma_deg, "reps": a.reps, "plane_bytes": int(3 * sum(m.size for m in masks))}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed = lift.pack(views, masks, orients, confs, "cuda")
    torch.cuda.synchronize()
    res["pack_upload_s"] = round(time.perf_counter() - t0, 3)
    dev = torch.from_numpy(pts).cuda()
    M, _, count = lift.moments_device(dev, packed)
    d0, _ = lift.solve_device(M, count)
    d, coherence, count = lift.directions_device(dev, packed, a.rounds, a.sigma_deg)
    res["views_used_median"] = int(np.median(count.cpu().numpy()))
    res["median_angle_deg_round_0"], _ = median_angle(d0.cpu().numpy(), truth)
    res["median_angle_deg_last_round"], res["points_with_a_direction"] = median_angle(d.cpu().numpy(), truth)
    res["median_coherence"] = round(float(np.median(coherence.cpu().numpy())), 4)
    m_ms = events(lambda: lift.moments_device(dev, packed), a.reps)
    r_ms = events(lambda: lift.moments_device(dev, packed, d0, s2), a.reps)
    s_ms = events(lambda: lift.solve_device(M, count), a.reps)
    l_ms = events(lambda: lift.directions_device(dev, packed, a.rounds, a.sigma_deg), a.reps)
    res.update({"moments_ms": round(m_ms, 3), "moments_with_prev_ms": round(r_ms, 3), "solve_ms": round(s_ms, 3),
                "directions_ms": round(l_ms, 3), "moments_point_views_per_s": round(a.points * a.views / m_ms * 1e3)})
    if not a.no_numpy:
        t0 = time.perf_counter()
        hd, _, hcount = lift.lift_directions(pts, views, masks, orients, confs, a.rounds, a.sigma_deg)
        dt = time.perf_counter() - t0
        hM = lift.moments_numpy(pts, views, masks, orients, confs)[0]
        res.update({"numpy_directions_s": round(dt, 2), "numpy_over_device": round(dt * 1e3 / l_ms, 1),
                    "numpy_median_angle_deg_last_round": median_angle(hd, truth)[0],
                    "moments_equal_bitwise": bool(hM.tobytes() == M.cpu().numpy().tobytes()),
                    "counts_equal": bool(np.array_equal(hcount, count.cpu().numpy()))})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
