"""Head meshes of the synthetic datasets (the reference's data/head_data.py), with a small OBJ reader in place of pytorch3d's
load_obj (not installed here).  Heads are grey (0.75, 0.75, 0.75, 1).  Normals: one per face -> every vertex of the face takes it
(the last face written wins), one per vertex -> as they are, any other count -> estimated from the vertices
(utils.normals.estimate_pointcloud_normals; normals_device = None: its host path, "cuda": its HIP kernels)."""
from typing import NamedTuple

import numpy as np

HEAD_COLOR = np.array([0.75, 0.75, 0.75, 1])


class HeadData(NamedTuple):
    verts: np.ndarray
    colors: np.ndarray
    normals: np.ndarray
    faces: np.ndarray


def load_obj(path):
    """(verts float32 [N, 3], faces int64 [F, 3], normals float32 [M, 3]) with pytorch3d load_obj's reading: `v` (x y z; extra
    values ignored), `vn`, and `f` with v, v/vt, v/vt/vn or v//vn corners; 1-based indices, negative ones counted from the end of
    the whole file's vertex list; polygons fanned into triangles (v0, v_i, v_i+1).  normals are every `vn` of the file."""
    verts, normals, faces = [], [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vn":
                normals.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                corner = [int(t.split("/")[0]) for t in tok[1:]]
                if len(corner) < 3:
                    raise ValueError(f"{path}: a face with fewer than 3 vertices: {line.strip()}")
                for k in range(1, len(corner) - 1):
                    faces.append([corner[0], corner[k], corner[k + 1]])
    v = np.array(verts, dtype=np.float32).reshape(-1, 3)
    f = np.array(faces, dtype=np.int64).reshape(-1, 3)
    f = np.where(f > 0, f - 1, f + v.shape[0])
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"{path}: a face index is out of range of the {v.shape[0]} vertices")
    return v, f, np.array(normals, dtype=np.float32).reshape(-1, 3)


def load_mesh(path):
    """(verts f64 [NV, 3], faces int64 [F, 3]) of a capture's head mesh, an OBJ or a triangle PLY (a `vertex` element with x, y, z and
    a `face` element whose list property holds three indices in every row); ValueError otherwise.  The drivers that read
    <scene>/head_mesh.ply (init_scalp.py, head_sdf.py) go through here and refuse in their own names."""
    import os
    if not os.path.exists(path):
        raise ValueError(f"{path} is missing (the head mesh; --mesh names another)")
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        verts, faces, _ = load_obj(path)
        return verts.astype(np.float64), faces
    if ext == ".ply":
        from utils.ply import read_ply
        els = dict(read_ply(path))
        if "vertex" not in els or "face" not in els or not all(n in els["vertex"].dtype.names for n in "xyz"):
            raise ValueError(f"{path}: a vertex element with x, y, z and a face element expected")
        vertex, face = els["vertex"], els["face"]
        lists = [n for n in face.dtype.names if face.dtype[n].shape]
        if len(lists) != 1 or face.dtype[lists[0]].shape != (3,):
            raise ValueError(f"{path}: faces of three vertices each expected (a triangle mesh)")
        return np.stack([vertex[n].astype(np.float64) for n in "xyz"], axis=1), face[lists[0]].astype(np.int64)
    raise ValueError(f"{path}: an .obj or a .ply mesh expected")


def _vertex_normals(verts, faces, normals, normals_device=None):
    if normals.shape[0] == faces.shape[0]:
        out = np.zeros((verts.shape[0], 3))
        out[faces.reshape(-1)] = np.repeat(normals, 3, axis=0)
        return out
    if normals.shape[0] != verts.shape[0]:
        from utils.normals import estimate_pointcloud_normals
        return estimate_pointcloud_normals(verts, device=normals_device)
    return normals


def load_head_from_usc_dataset(file_path, normal_required=False, normals_device=None):
    verts, faces, normals = load_obj(file_path)
    return HeadData(verts=verts, colors=np.tile(HEAD_COLOR, (verts.shape[0], 1)),
                    normals=_vertex_normals(verts, faces, normals, normals_device) if normal_required else None, faces=faces)


def load_head_from_cy_dataset(file_path, normals_device=None):
    from data.hair_data import zup_to_yup
    verts, faces, normals = load_obj(file_path)
    verts = 0.25 * verts.astype(np.float64) / 100
    verts = (zup_to_yup() @ verts.T).T
    return HeadData(verts=verts, colors=np.tile(HEAD_COLOR, (verts.shape[0], 1)),
                    normals=_vertex_normals(verts, faces, normals, normals_device), faces=faces)


head_data_load_callbacks = {"usc_hair_salon": load_head_from_usc_dataset, "cem_yuksel": load_head_from_cy_dataset}
