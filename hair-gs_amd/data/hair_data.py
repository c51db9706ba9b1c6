"""Ground-truth strands of the synthetic datasets in one container (the reference's data/hair_data.py): what the dataset
synthesis renders (synthesize.py) and what evaluation compares with (hair_eval_data.npz).

USC-HairSalon .data: int32 strand count (must be 10000), then per strand an int32 vertex count (1 or 100) and that many float32
xyz.  Cem Yuksel .hair: data/cy_hair.py; the segment counts are taken as POINT counts per strand, as the reference takes them, and
the strands are scaled by 0.25 / 100 and turned from z-up to y-up.  Strands are kept when i % load_freq == 0, load_freq =
num_strands // int(num_strands * pct_strands / 100); USC strands with one vertex are skipped."""
import struct
from typing import NamedTuple

import numpy as np

from data.cy_hair import read_cy_hair

USC_PALETTE = np.array([[0.545, 0.271, 0.075, 1], [0.639, 0.341, 0.125, 1], [0.561, 0.388, 0.196, 1]])
CY_PALETTE = np.array([[1.0, 0.85, 0.47, 1], [0.76, 0.75, 0.65, 1], [0.95, 0.8, 0.53, 1]])


class HairData(NamedTuple):
    verts: np.ndarray
    colors: np.ndarray
    normals: np.ndarray
    edges: np.ndarray
    strand_root_idx: np.ndarray
    verts_id_to_strand_id: np.ndarray


def hsv2rgb_u8(h, s=255, v=255):
    """OpenCV's 8-bit COLOR_HSV2RGB of one pixel (hue 0..180, wrapping at 180): float32 h * (6 / 180), sector = floor(h),
    f = h - sector, tab = (v, v (1 - s), v (1 - s f), v (1 - s (1 - f))) with s, v scaled to [0, 1], the sector's permutation, and
    every channel rounded half to even from x * 255 and saturated.  Returns uint8 [3] (R, G, B)."""
    f32 = np.float32
    hh = f32(int(h)) * (f32(6.0) / f32(180.0))
    ss, vv = f32(int(s)) * (f32(1.0) / f32(255.0)), f32(int(v)) * (f32(1.0) / f32(255.0))
    if ss == 0:
        b = g = r = vv
    else:
        while hh < 0:
            hh = f32(hh + f32(6.0))
        while hh >= 6:
            hh = f32(hh - f32(6.0))
        sector = int(np.floor(hh))
        hh = f32(hh - f32(sector))
        if not 0 <= sector < 6:
            sector, hh = 0, f32(0.0)
        tab = (vv, f32(vv * f32(f32(1.0) - ss)), f32(vv * f32(f32(1.0) - f32(ss * hh))), f32(vv * f32(f32(1.0) - f32(ss * f32(f32(1.0) - hh)))))
        perm = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))[sector]    # (b, g, r)
        b, g, r = tab[perm[0]], tab[perm[1]], tab[perm[2]]
    return np.array([np.clip(np.rint(f32(x * f32(255.0))), 0, 255) for x in (r, g, b)], dtype=np.uint8)


def _strand_color(i, palette, hues, hsv):
    if hsv:
        return np.append(hsv2rgb_u8(np.uint8(hues[i])) / 255, 1)
    return palette[i % palette.shape[0]]


def _finish(strands, colors, normals, edges, roots, ids):
    return HairData(verts=np.concatenate(strands, axis=0), colors=np.concatenate(colors, axis=0), normals=normals,
                    edges=np.concatenate(edges, axis=0), strand_root_idx=np.array(roots),
                    verts_id_to_strand_id=np.concatenate(ids, axis=0))


def _append(strands, edges, colors, roots, ids, xyz, color, last):
    n = xyz.shape[0]
    roots.append(last)
    strands.append(xyz)
    edges.append(np.column_stack([np.arange(last, last + n - 1), np.arange(last + 1, last + n)]).astype(np.uint32))
    ids.append(np.full(n, len(strands) - 1, dtype=np.uint32))
    colors.append(np.tile(color, (n, 1)) if np.ndim(color) == 1 else color)
    return last + n


def load_hair_from_usc_dataset(file_path, normal_required=False, hsv_spectre_color=True, pct_strands=100, normals_device=None):
    """normals_device: None = the host path of utils.normals, "cuda" = its HIP kernels."""
    with open(file_path, "rb") as fh:
        buf = fh.read()
    (num_strands,) = struct.unpack_from("<i", buf, 0)
    load_freq = num_strands // int(num_strands * pct_strands / 100)
    assert num_strands == 10000, f"Expected 10000 strands, got: {num_strands}"
    hues = np.linspace(start=0, stop=180, num=num_strands)
    strands, edges, colors, roots, ids = [], [], [], [], []
    pos, last = 4, 0
    for i in range(num_strands):
        (nv,) = struct.unpack_from("<i", buf, pos)
        pos += 4
        assert nv == 1 or nv == 100, f"Num_verts should be 1 or 100, got: {nv}"
        xyz = np.frombuffer(buf, dtype="<f4", count=3 * nv, offset=pos).reshape(nv, 3).astype(np.float64)
        pos += 12 * nv
        if i % load_freq != 0 or nv == 1:
            continue
        last = _append(strands, edges, colors, roots, ids, xyz, _strand_color(i, USC_PALETTE, hues, hsv_spectre_color), last)
    normals = None
    if normal_required:
        from utils.normals import estimate_pointcloud_normals
        normals = estimate_pointcloud_normals(np.concatenate(strands, axis=0), device=normals_device)
    return _finish(strands, colors, normals, edges, roots, ids)


def zup_to_yup():
    """The reference's rotation of the Cem Yuksel models: R_y(-90 deg) R_x(-90 deg)."""
    from scipy.spatial.transform import Rotation
    return Rotation.from_euler("y", -90, degrees=True).as_matrix() @ Rotation.from_euler("x", -90, degrees=True).as_matrix()


def load_hair_from_cy_dataset(file_path, hsv_spectre_color=True, pct_strands=100):
    hf = read_cy_hair(file_path)
    all_points = np.asarray(hf.points, dtype=np.float64).reshape(-1, 3)
    num_strands = hf.header.hair_count
    if hf.segments is None:
        strand_points = np.full(num_strands, int(all_points.shape[0] / (3 * num_strands)), dtype=np.int32)
    else:
        strand_points = np.asarray(hf.segments, dtype=np.int64)
    raw_colors = None if hf.colors is None else np.asarray(hf.colors, dtype=np.float64)
    load_freq = num_strands // int(num_strands * pct_strands / 100)
    hues = np.linspace(start=0, stop=180, num=num_strands)
    strands, edges, colors, roots, ids, dirs = [], [], [], [], [], []
    start, last = 0, 0
    for i in range(num_strands):
        n = int(strand_points[i])
        s0, start = start, start + n
        if i % load_freq != 0:
            continue
        xyz = all_points[s0:s0 + n]
        d = np.concatenate([xyz[1:] - xyz[:-1], np.array([[0.0, 0.0, 1.0]])], axis=0)
        dirs.append(d / np.linalg.norm(d, axis=1, keepdims=True))
        if raw_colors is None or hsv_spectre_color:
            color = _strand_color(i, CY_PALETTE, hues, hsv_spectre_color)
        else:                                   # (per-point file colours, alpha 1)
            color = np.column_stack([raw_colors[s0:s0 + n], np.ones(n)])
        last = _append(strands, edges, colors, roots, ids, xyz, color, last)
    hair = _finish(strands, colors, np.concatenate(dirs, axis=0), edges, roots, ids)
    verts = 0.25 * hair.verts / 100                 # cm -> m, scaled to a 0.17 m head
    verts = (zup_to_yup() @ verts.T).T
    return hair._replace(verts=verts)


def save_hair_eval_data_npz(file_path, hair):
    """hair_eval_data.npz of a HairData (read by data.eval_data.load_hair_eval_data_npz): points = the first vertex of every
    edge, directions = the unit edge vectors, points_id_to_strand_id of those vertices, and edges = the edges whose end starts
    another edge (each strand's last segment removed), renumbered over the vertices they use."""
    seg = hair.verts[hair.edges]
    directions = seg[:, 1] - seg[:, 0]
    directions = directions / np.linalg.norm(directions, axis=1, keepdims=True)
    points = hair.verts[hair.edges[:, 0]]
    sid = hair.verts_id_to_strand_id[hair.edges[:, 0]]
    edges = hair.edges[np.isin(hair.edges[:, 1], hair.edges[:, 0])]
    old = np.unique(edges)
    mapping = np.zeros(int(old.max()) + 1 if old.size else 1, dtype=np.int64)
    mapping[old] = np.arange(old.shape[0])
    np.savez(file_path, points=points, directions=directions, points_id_to_strand_id=sid, edges=mapping[edges])


hair_data_load_callbacks = {"usc_hair_salon": load_hair_from_usc_dataset, "cem_yuksel": load_hair_from_cy_dataset}
