"""Meshes, cameras, masks and the small scene shared by tests/test_scalp_cpu.py and tests/test_scalp_gpu.py (cameras and masks come
from tests/carve_cases.py)."""
import os

import numpy as np

from tests import carve_cases as CC

INF, NAN = float("inf"), float("nan")
MIN_COS, DEPTH_TOL = 0.25, 0.02                    # the labelled cap's knobs
BALL_CENTRE, BALL_RADIUS = np.array([1.7, 0.3, 0.3]), 0.45


def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(verts f64 [10*4^s + 2, 3], faces int64 [20*4^s, 3]), counter-clockwise seen from outside."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
             (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in verts]
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
    return np.asarray(centre, np.float64) + radius * np.array(verts), np.array(faces, np.int64)


def cap_views():
    """Eight ring cameras of two sizes and one camera above the head."""
    return CC.ring_views(8, radius=3, sizes=((96, 80), (128, 96)), f_scale=1.1) + \
        [CC.view(*CC.look_at((0.3, 0.2, 3.2)), 128, 96, 140.0, name="top.png")]


def cap_mask(v, z_min=0.25):
    """uint8 [H, W]: set where the ray through the pixel's centre first meets the unit sphere at z > z_min."""
    C = -(v.R.T @ v.t)
    xs = (np.arange(v.W, dtype=np.float64) + 0.5 - v.cx) / v.fx
    ys = (np.arange(v.H, dtype=np.float64) + 0.5 - v.cy) / v.fy
    d = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.ones((v.H, v.W))), axis=-1) @ v.R     # rows: R^T d
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    b = d @ C
    disc = b * b - (C @ C - 1.0)
    s = -b - np.sqrt(np.maximum(disc, 0.0))
    z = C[2] + s * d[..., 2]
    return np.where((disc > 0.0) & (s > 0.0) & (z > z_min), 255, 0).astype(np.uint8)


def head_and_ball():
    """The unit head (3 subdivisions) and a ball of 2 subdivisions beside it, as one mesh; n_head = the head's vertex count."""
    hv, hf = icosphere(3)
    bv, bf = icosphere(2, BALL_RADIUS, BALL_CENTRE)
    return np.concatenate([hv, bv]), np.concatenate([hf, bf + hv.shape[0]]), hv.shape[0]


def _at(depth, *uv):
    """World points of an identity view that land on the image points uv at `depth` (depth a power of two: u = x/depth exactly)."""
    return [(u * depth, v * depth, depth) for u, v in uv]


def edge_faces():
    """[(name, verts [3], expectation)] under carve_cases.identity_view(W, H) with W >= 8 and H >= 6.  The expectation is
    ("dropped",) or a dict {(py, px): z} of the covered centres, every other pixel +inf; "frame": every pixel holds that value."""
    cases = [
        ("corner box holds no centre", _at(1.0, (0.6, 0.6), (0.9, 0.6), (0.6, 0.9)), {}),
        ("sliver passes beside its box's only centre", _at(1.0, (0.6, 0.6), (2.4, 2.45), (0.6, 0.65)), {}),
        ("exactly one centre", _at(1.0, (1.2, 1.2), (1.9, 1.3), (1.4, 1.9)), {(1, 1): 1.0}),
        ("vertex on a centre", _at(2.0, (1.5, 1.5), (1.9, 1.6), (1.6, 1.9)), {(1, 1): 2.0}),
        ("shared edge, near side", _at(2.0, (0.5, 0.5), (3.5, 3.5), (3.5, 0.5)), {(py, px): 2.0 for py in range(4) for px in range(py, 4)}),
        ("shared edge, far side", _at(4.0, (0.5, 0.5), (3.5, 3.5), (0.5, 3.5)), {(py, px): 4.0 for py in range(4) for px in range(py + 1)}),
        ("larger than the frame", _at(2.0, (-100.0, -100.0), (300.0, -100.0), (-100.0, 300.0)), {"frame": 2.0}),
        ("a vertex behind the camera", [(1.0, 1.0, 1.0), (3.0, 1.0, 1.0), (1.0, 3.0, -1.0)], ("dropped",)),
        ("a vertex on the camera plane", [(1.0, 1.0, 1.0), (3.0, 1.0, 1.0), (1.0, 3.0, 0.0)], ("dropped",)),
        ("degenerate", _at(1.0, (0.5, 0.5), (2.5, 2.5), (1.5, 1.5)), {}),
        ("a NaN vertex", [(1.0, 1.0, 1.0), (3.0, NAN, 1.0), (1.0, 3.0, 1.0)], ("dropped",)),
        ("an infinite vertex", [(1.0, 1.0, 1.0), (INF, 1.0, 1.0), (1.0, 3.0, 1.0)], ("dropped",)),
        ("one pixel row", _at(2.0, (0.2, 4.4), (40.3, 4.45), (0.2, 4.6)), "row"),
    ]
    return cases


def edge_mesh(names=None, flip=False):
    """The edge cases (all, or those named) as one mesh: (verts [3n, 3], faces [n, 3])."""
    tris = [t for name, t, _ in edge_faces() if names is None or name in names]
    verts = np.array([p for t in tris for p in t], np.float64).reshape(-1, 3)
    faces = np.arange(verts.shape[0], dtype=np.int64).reshape(-1, 3)
    return verts, faces[:, ::-1].copy() if flip else faces


def random_faces(n, seed=0, centre=(0.0, 0.0, 0.3), spread=0.8, size=0.15):
    """n small triangles around `centre`: (verts [3n, 3], faces [n, 3])."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64) + rng.normal(scale=spread, size=(n, 1, 3))
    verts = (c + rng.normal(scale=size, size=(n, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int64).reshape(-1, 3)


def join(*meshes):
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, np.float64).reshape(-1, 3))
        faces.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += verts[-1].shape[0]
    return np.concatenate(verts), np.concatenate(faces)


def write_obj(path, verts, faces):
    with open(path, "w") as fh:
        for v in verts:
            fh.write(f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
        for f in faces:
            fh.write(f"f {int(f[0]) + 1} {int(f[1]) + 1} {int(f[2]) + 1}\n")


def write_ply(path, verts, faces):
    from utils.ply import table, write_ply as write
    face = np.empty(faces.shape[0], dtype=[("vertex_indices", "<i4", (3,))])
    face["vertex_indices"] = faces
    write(path, [("vertex", table(np.asarray(verts, np.float32), ["x", "y", "z"])), ("face", face)])


def build_scene(root, model="PINHOLE", mesh="ply"):
    """A capture under <root>: carve_cases.build_scene's six axis cameras at distance 10 (64 x 64, f = 200) around the unit head, masks
    of the cap z > 0.25, and the head as head_mesh.ply (or .obj).  Returns (views, masks, verts, faces) -- verts as the file holds
    them, float32 values."""
    from PIL import Image as PILImage
    views, _, _, _ = CC.build_scene(root, r=1.0, model=model)
    raw = CC.axis_views(10.0)
    masks = [cap_mask(v) for v in raw]
    for v, m in zip(raw, masks):
        PILImage.fromarray(m).save(os.path.join(root, "masks", v.name))
    verts, faces = icosphere(2)
    verts = verts.astype(np.float32).astype(np.float64)
    if mesh == "ply":
        write_ply(os.path.join(root, "head_mesh.ply"), verts, faces)
    else:
        write_obj(os.path.join(root, "head_mesh.obj"), verts, faces)
    return views, masks, verts, faces
