"""Input files for the dataset synthesis tests: a USC-HairSalon strand file and a sphere head (OBJ) written here."""
import struct

import numpy as np


def write_usc(path, n_long=100, seed=0, n_verts=100):
    """10000 strands: every (10000 // n_long)-th one has n_verts vertices (random walks from a 0.1 m sphere), the others one."""
    import synthetic
    step = 10000 // n_long
    walks = synthetic.strand_polylines(n_long, n_verts - 1, seed=seed)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", 10000))
        for i in range(10000):
            if i % step == 0 and i // step < n_long:
                fh.write(struct.pack("<i", n_verts))
                fh.write(walks[i // step].astype("<f4").tobytes())
            else:
                fh.write(struct.pack("<i", 1))
                fh.write(np.array([0.0, 0.3, 0.0], "<f4").tobytes())
    return walks


def sphere_mesh(r=0.085, n_lat=32, n_lon=64):
    """Closed sphere around the origin, counter-clockwise faces seen from outside, outward vertex normals."""
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.ones_like(lon)[None],
                     -np.sin(lat)[:, None] * np.sin(lon)[None]], -1).reshape(-1, 3)
    n = np.concatenate([[[0, 1, 0]], ring, [[0, -1, 0]]])
    idx = lambda a, b: 1 + a * n_lon + (b % n_lon)
    f = []
    for b in range(n_lon):
        f.append([0, idx(0, b), idx(0, b + 1)])
        f.append([len(n) - 1, idx(n_lat - 2, b + 1), idx(n_lat - 2, b)])
        for a in range(n_lat - 2):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    f = np.array(f)
    v = n * r
    c = v[f].mean(1)
    flip = (np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) * c).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f, n


def write_obj(path, v, f, vn=None):
    with open(path, "w") as fh:
        for p in v:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for p in (vn if vn is not None else []):
            fh.write(f"vn {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for t in f:
            fh.write("f " + " ".join(f"{k + 1}//{k + 1}" if vn is not None else f"{k + 1}" for k in t) + "\n")
