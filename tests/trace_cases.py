"""Clouds, fields and roots shared by tests/test_trace_cpu.py and tests/test_trace_gpu.py: the smallest at which the kernels of
csrc/hgs_trace.hip can go wrong.  Spacing, origin and radius are dyadic, so that `on a node` and `d2 == r2` are exact statements."""
import numpy as np

GRIDS = {"g2": (2, 2, 2), "g543": (5, 4, 3), "g1796": (17, 9, 6)}      # (nx, ny, nz): the second and third are not cubic
H = 0.25
ORIGIN = np.array([-0.5, 0.25, 1.0])
R = 0.375                                                               # 1.5 spacings
NS = (0, 1, 63, 64, 65, 257)
SS = (0, 1, 63, 64, 65, 300)
DENORMAL = 5e-324


def node(shape, ix, iy, iz):
    return ORIGIN + H * np.array([ix, iy, iz], np.float64)


def special_points(shape):
    """(points, dirs, n_skipped): points on nodes, one at exactly d2 == r2 from a node, points up to and beyond r outside every
    face, coincident points, and the directions that are skipped (zero, NaN, infinite, denormal: its square underflows to 0) next to
    a point that is not finite."""
    nx, ny, nz = shape
    top = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    pts, dirs = [], []
    d_generic = np.array([0.3, -0.5, 0.8])
    for c in ((0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, nz - 1), (1, 1, 1)):
        pts.append(node(shape, *c))                                      # on a node: d2 == 0, k == 1
        dirs.append(d_generic)
    pts.append(node(shape, 1, 1, 1) + np.array([R, 0.0, 0.0]))           # d2 == r2 exactly from node (1, 1, 1): excluded there
    dirs.append(np.array([0.0, 2.0, 0.0]))
    for a in range(3):
        for side in (0, 1):
            for out in (0.5 * R, R - 2.0 ** -30, R, R + 2.0 ** -30, 3.0 * R, 40.0):
                t = np.floor(0.5 * top)                                  # (on a node in the other two axes)
                t[a] = top[a] if side else 0.0
                p = ORIGIN + H * t
                p[a] += out if side else -out
                pts.append(p)
                dirs.append(np.roll(d_generic, a))
    pts += [node(shape, 0, 1, 0) + 0.1] * 3                               # coincident
    dirs += [np.array([1.0, 1.0, 0.0]), np.array([-1.0, -1.0, 0.0]), np.array([0.0, 0.0, 3.0])]
    bad = [np.zeros(3), np.array([np.nan, 1.0, 0.0]), np.array([np.inf, 0.0, 0.0]), np.array([DENORMAL, 0.0, -DENORMAL]),
           np.array([1e200, 1e200, 0.0])]                                 # (the last: dot overflows)
    for b in bad:
        pts.append(node(shape, 0, 0, 0) + 0.05)
        dirs.append(b)
    for b in (np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0]), np.array([0.0, 0.0, -np.inf])):
        pts.append(ORIGIN + b)
        dirs.append(d_generic)
    pts.append(np.array([1e300, -1e300, 1e300]))                          # finite, far outside: (x - origin)*k overflows
    dirs.append(d_generic)
    return np.array(pts), np.array(dirs), len(bad) + 3


def cloud(shape, n, seed=0):
    """(points, dirs) f64 [n, 3]: the special points first (when n allows), then a random cloud over the grid and a margin around it."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    sp, sd, _ = special_points(shape)
    m = max(n, sp.shape[0])
    lo, hi = ORIGIN - 2 * R, ORIGIN + H * (np.array([nx, ny, nz]) - 1) + 2 * R
    pts = np.concatenate([sp, rng.uniform(lo, hi, size=(m, 3))])
    dirs = np.concatenate([sd, rng.normal(size=(m, 3)) * rng.uniform(0.01, 100.0, size=(m, 1))])
    return np.ascontiguousarray(pts[:n]), np.ascontiguousarray(dirs[:n])


def pile(shape, n=300):
    """n points on and around one node: every one of them adds to it."""
    rng = np.random.default_rng(4)
    c = node(shape, shape[0] // 2, shape[1] // 2, shape[2] // 2)
    pts = c[None, :] + rng.uniform(-0.2 * H, 0.2 * H, size=(n, 3))
    pts[::3] = c
    return pts, rng.normal(size=(n, 3))


def combed(shape, n, seed=2):
    """A cloud whose directions are a smooth field with noise: its nodes have a clear top eigenvector (the solve tests)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    pts = rng.uniform(ORIGIN, ORIGIN + H * (np.array([nx, ny, nz]) - 1), size=(n, 3))
    d = np.stack([np.cos(pts[:, 1] * 2.0), np.sin(pts[:, 1] * 2.0), 0.3 * np.cos(pts[:, 0])], axis=1) + 0.15 * rng.normal(size=(n, 3))
    return pts, d * np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]      # (lines, not vectors: the sign is arbitrary)


def hard_sums():
    """int64 [8, 7] (W, xx, xy, xz, yy, yz, zz): empty, W == 0 with entries, isotropic, rank 1, two equal top eigenvalues, huge, tiny,
    and one generic row."""
    one = 1 << 32
    e = np.array([0.6, 0.0, 0.8])
    o = np.rint(np.outer(e, e) * one).astype(np.int64)
    return np.array([[0] * 7,
                     [0, one, 0, 0, 2 * one, 0, 3 * one],
                     [one, one, 0, 0, one, 0, one],
                     [one, o[0, 0], o[0, 1], o[0, 2], o[1, 1], o[1, 2], o[2, 2]],
                     [one, 2 * one, 0, 0, 2 * one, 0, one],
                     [1 << 56, 1 << 55, 1 << 53, 0, 1 << 54, -(1 << 52), 1 << 53],
                     [1, 3, 1, 0, 2, 0, 1],
                     [5 * one, 3 * one, one // 3, -one // 5, 2 * one, one // 7, one]], np.int64)


# ---- fields for the trace ------------------------------------------------------------------------------------------------
TRACE_SHAPE = GRIDS["g1796"]
STEP = 0.5 * H


def _nodes(shape):
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return x, y, z


def uniform_field(d=(1.0, 0.0, 0.0), shape=TRACE_SHAPE):
    from utils.trace import Field
    nx, ny, nz = shape
    d = np.asarray(d, np.float64)
    return Field(ORIGIN, H, shape, np.broadcast_to(d / np.linalg.norm(d), (nz, ny, nx, 3)).copy(), np.ones((nz, ny, nx)))


CENTRE = (8.3, 4.2)                # of the circular field, in node units: on no node and on no line of nodes


def circular_field(core=1.2, flip=False, shape=TRACE_SHAPE):
    """Tangent directions around the z axis through CENTRE, confidence 2, an empty core; flip: every second node's dir negated."""
    from utils.trace import Field
    x, y, z = _nodes(shape)
    rx, ry = x - CENTRE[0], y - CENTRE[1]
    rr = np.sqrt(rx * rx + ry * ry)
    d = np.stack([-ry / rr, rx / rr, np.zeros_like(rr)], axis=-1)
    conf = np.where(rr < core, 0.0, 2.0)
    d[conf == 0] = 0.0
    if flip:
        odd = ((x + y + z) % 2 == 1)
        d[odd] = -d[odd]
    return Field(ORIGIN, H, shape, d, conf)


def half_spaces(shape=TRACE_SHAPE):
    """+x for ix < 8, +y from there on: 90 degrees apart."""
    from utils.trace import Field
    x, y, z = _nodes(shape)
    d = np.where((x < 8)[..., None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    return Field(ORIGIN, H, shape, d, np.ones(x.shape))


def slab_field(lo=4, hi=5, shape=TRACE_SHAPE):
    """+x everywhere, confidence 0 at the nodes lo <= ix <= hi."""
    f = uniform_field(shape=shape)
    f.conf[:, :, lo:hi + 1] = 0.0
    return f


def at(tx, ty, tz):
    """The position with node coordinates t (dyadic t: exact)."""
    return ORIGIN + H * np.array([tx, ty, tz], np.float64)


def roots(n, seed=6, shape=TRACE_SHAPE):
    """(roots, p0) f64 [n, 3]: a NaN root, roots outside the grid and on its last node first, then random roots in and around the
    grid with random unit directions."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    special = np.array([[np.nan, 0.5, 1.2], at(-0.5, 2, 2), at(nx - 1, 3, 2), at(3, ny - 1, 2), at(3, 3, nz - 1), at(0, 0, 0), [1e300, 0.0, 0.0],
                        [np.inf, 0.5, 1.2]])
    m = max(n, special.shape[0])
    r = np.concatenate([special, rng.uniform(at(-0.3, -0.3, -0.3), at(nx - 0.7, ny - 0.7, nz - 0.7), size=(m, 3))])
    p = rng.normal(size=(r.shape[0], 3))
    p[:, 2] *= 0.3
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return np.ascontiguousarray(r[:n]), np.ascontiguousarray(p[:n])


KNOBS = dict(step=STEP, max_steps=48, cos_max=0.5, min_conf=0.5, max_gap=4)


# ---- a synthetic scene for the driver -----------------------------------------------------------------------------------------
def write_scene(root, n_points=6000, n_roots=120, directions=True, head=True, seed=0):
    """A capture directory (tests/test_dataset_io_cpu.py's two 64 x 64 views) whose points3D.ply is a combed shell over the upper half
    of a head of radius 0.5: hair lines that run down the meridians, between radius 0.5 and 0.85; the scalp points lie on the head."""
    from data.dataset_readers import storePly
    from tests.test_dataset_io_cpu import _write_capture
    _write_capture(root, n_views=2, W=64, H=64)
    rng = np.random.default_rng(seed)

    def upper(n, r_lo, r_hi, z_min):
        v = rng.normal(size=(4 * n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v = v[v[:, 2] > z_min][:n]
        return v * rng.uniform(r_lo, r_hi, size=(v.shape[0], 1))
    pts = upper(n_points, 0.5, 0.85, -0.2)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    down = np.array([0.0, 0.0, -1.0])[None, :] - radial * (-radial[:, 2:3])            # -z projected on the tangent plane
    down += np.array([0.2, 0.0, 0.0])                                                   # (a little sideways: defined at the pole too)
    normals = (down / np.linalg.norm(down, axis=1, keepdims=True)).astype(np.float32)
    normals[::10] = 0.0                                                                 # points without a direction
    ply = root / "sparse" / "0" / "points3D.ply"
    storePly(str(ply), pts.astype(np.float32), np.full((pts.shape[0], 3), 128, np.uint8), normals if directions else None)
    if head:
        hv = rng.normal(size=(400, 3))
        hv = 0.5 * hv / np.linalg.norm(hv, axis=1, keepdims=True)
        np.savez(root / "head_reconstruction_data.npz", head_verts=hv, scalp_verts=upper(n_roots, 0.5, 0.5, 0.3))
    return pts, normals
