"""Kind patterns, tensors and a synthetic capture shared by tests/test_fill_cpu.py and tests/test_fill_gpu.py: the smallest at which
csrc/hgs_fill.hip can go wrong.  The grids, the origin and the spacing are tests/trace_cases.py's."""
import numpy as np

from tests import trace_cases as TC

OUT, FREE, FIXED = 0, 1, 2
GRIDS = TC.GRIDS
PATTERNS = ("thirds", "all_free", "isolated", "borders", "middle", "negative", "minus_zero")
SWEEPS_CPU = (0, 1, 2, 7)
SWEEPS_GPU = (0, 1, 2, 7, 64)
FREE_COUNTS = (0, 1, 63, 64, 65, 257, 918)               # of the 17 x 9 x 6 grid's 918 nodes


def unit_dirs(shape, seed):
    nx, ny, nz = shape
    d = np.random.default_rng(seed).normal(size=(nz, ny, nx, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def field_of(dirs, kind, shape):
    """A Field whose conf is 1 at the FIXED nodes and 0 elsewhere: classify(field, 0.5, kind != OUT) gives `kind` back."""
    from utils.trace import Field
    return Field(TC.ORIGIN, TC.H, shape, dirs, (kind == FIXED).astype(np.float64))


def pattern(name, shape):
    """(dirs f64 [nz, ny, nx, 3], kind uint8 [nz, ny, nx], T f64 [6, nz, ny, nx]): T is the seed, except where the pattern says so."""
    from utils import field_fill as FF
    nx, ny, nz = shape
    rng = np.random.default_rng(sum(map(ord, name)) + nx)
    dirs = unit_dirs(shape, 7 + nx)
    mid = (nz // 2, ny // 2, nx // 2)
    extra = None
    if name == "thirds":
        kind = rng.integers(0, 3, size=(nz, ny, nx)).astype(np.uint8)
    elif name == "all_free":                               # nothing FIXED: stays +0.0
        kind = np.full((nz, ny, nx), FREE, np.uint8)
    elif name == "isolated":                               # the FREE node (0, 0, 0) has three neighbours off the grid and three OUT: c = 0
        kind = rng.integers(0, 3, size=(nz, ny, nx)).astype(np.uint8)
        kind[0, 0, 0] = FREE
        kind[0, 0, 1] = kind[0, 1, 0] = kind[1, 0, 0] = OUT
        extra = ((slice(None), 0, 0, 0), np.array([0.25, -0.5, 0.125, 0.5, -0.0, 0.25]))       # a value to keep, not the seed's 0
    elif name == "borders":                                # every corner, edge and face node is FREE
        kind = rng.integers(0, 3, size=(nz, ny, nx)).astype(np.uint8)
        kind[[0, -1]], kind[:, [0, -1]], kind[:, :, [0, -1]] = FREE, FREE, FREE
        kind.reshape(-1)[1] = FIXED                        # (a 2 x 2 x 2 grid is all border: something to diffuse from)
    elif name in ("middle", "negative", "minus_zero"):     # one FIXED node in the middle
        kind = np.full((nz, ny, nx), FREE, np.uint8)
        kind[mid] = FIXED
        if name == "negative":
            dirs[mid] = np.array([-0.6, 0.0, -0.8])
        if name == "minus_zero":                           # its products are -0.0: a neighbour's sum 0.0 + -0.0 is +0.0
            dirs[mid] = np.array([1.0, -0.0, 0.0])
    else:
        raise KeyError(name)
    T = FF.seed(field_of(dirs, kind, shape), kind)
    if extra is not None:
        T[extra[0]] = extra[1]
    return dirs, kind, T


def counted(F, shape=GRIDS["g1796"]):
    """(dirs, kind, T) with exactly F FREE nodes, FREE nodes on every face of the grid where F allows; the others FIXED or OUT at random."""
    from utils import field_fill as FF
    nx, ny, nz = shape
    rng = np.random.default_rng(100 + F)
    nodes = nx * ny * nz
    kind = rng.integers(0, 2, size=nodes).astype(np.uint8) * FIXED            # OUT or FIXED
    faces = [0, nodes - 1, nx - 1, nx * ny - 1, nx * (ny - 1), nodes - nx * ny]   # corners: together they touch all six faces
    order = np.concatenate([faces, rng.permutation(np.setdiff1d(np.arange(nodes), faces))])
    kind[order[:F]] = FREE
    kind = kind.reshape(nz, ny, nx)
    dirs = unit_dirs(shape, 11)
    return dirs, kind, FF.seed(field_of(dirs, kind, shape), kind)


def wall(left=(1.0, 0.0, 0.0), right=(0.0, 1.0, 0.0), shape=GRIDS["g1796"]):
    """Two FIXED regions (the planes ix = 0 and ix = nx - 1) with different directions, a full plane of OUT nodes at ix = 8 between
    them; everything else FREE."""
    nx, ny, nz = shape
    kind = np.full((nz, ny, nx), FREE, np.uint8)
    kind[:, :, 0] = kind[:, :, -1] = FIXED
    kind[:, :, 8] = OUT
    dirs = np.zeros((nz, ny, nx, 3))
    dirs[:, :, 0], dirs[:, :, -1] = np.asarray(left, np.float64), np.asarray(right, np.float64)
    return dirs, kind


LINE_SHAPE = (9, 2, 2)
LINE_SWEEPS = 400


def line():
    """(field, kind): a 9 x 2 x 2 grid in which only the line y = z = 0 is not OUT; its ends are FIXED with e_x and e_y, the seven
    nodes between them FREE."""
    nx, ny, nz = LINE_SHAPE
    kind = np.zeros((nz, ny, nx), np.uint8)
    kind[0, 0, :] = FREE
    kind[0, 0, 0] = kind[0, 0, -1] = FIXED
    dirs = np.zeros((nz, ny, nx, 3))
    dirs[0, 0, 0], dirs[0, 0, -1] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    return field_of(dirs, kind, LINE_SHAPE), kind


def check_line(T, d, conf):
    """The analytic line's bounds: after 400 sweeps the 1-D Jacobi error, which shrinks by cos(pi/8) < 0.924 a sweep, is below
    0.924^400 < 1e-13."""
    i = np.arange(9, dtype=np.float64)
    want = np.zeros((6, 9))
    want[0], want[3] = 1.0 - i / 8.0, i / 8.0
    assert np.abs(T[:, 0, 0, :] - want).max() <= 1e-12
    assert not T[:, 1].any() and not T[:, :, 1].any()                          # the OUT nodes
    assert np.abs(conf[0, 0] - np.abs(1.0 - i / 4.0)).max() <= 1e-9
    for k in range(9):
        if k != 4:                                                             # (i = 4 is degenerate: Txx == Tyy)
            assert np.abs(d[0, 0, k] - ((1.0, 0.0, 0.0) if k < 4 else (0.0, 1.0, 0.0))).max() <= 1e-9, k


# ---- a synthetic capture for the driver ------------------------------------------------------------------------------------------
# The gap and the sweeps were chosen on the numpy path, before any assertion ran, so that the two conditions of
# test_fill_cpu.test_driver_fills_the_gap hold with room to spare: at --grid 28 the spacing is about 0.1, so a shell from 0.95 on
# leaves 4.5 voxels to the head of radius 0.5, of which the splat radius covers 1.5 and --max_gap 4 half-voxel steps 2 (shells from 0.9
# on already left no strand; 0.85 left 13 of 120); 60 sweeps are about three times the gap's square (30 gave the same strands).  The
# hair lines leave the head at 45 degrees (LIFT: as much outward as down the meridian): where the visible hair lies flat on the head
# the filled direction turns by 90 degrees where the radial and the tangential tensor cross, and the tracer's --max_angle 60 stops there.
HEAD_R, SHELL, LIFT = 0.5, (0.95, 1.1), 1.0
FILL = 60
ROOTS = 120


def write_scene(root, shell=SHELL, lift=LIFT, n_points=6000, n_roots=ROOTS, sdf=True, seed=0):
    """tests/trace_cases.write_scene's capture with the combed shell moved out to `shell` (a gap between it and the head of radius
    0.5 that the scalp points lie on) and head_sdf.npz built from a small sphere mesh (masks/ holds that capture's random masks)."""
    from data.dataset_readers import storePly
    from tests import head_sdf_cases as HC
    from tests.test_dataset_io_cpu import _write_capture
    from utils import head_sdf as H
    _write_capture(root, n_views=2, W=64, H=64)
    rng = np.random.default_rng(seed)

    def upper(n, r_lo, r_hi, z_min):
        v = rng.normal(size=(4 * n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v = v[v[:, 2] > z_min][:n]
        return v * rng.uniform(r_lo, r_hi, size=(v.shape[0], 1))
    pts = upper(n_points, shell[0], shell[1], -0.2)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    down = np.array([0.0, 0.0, -1.0])[None, :] + radial * radial[:, 2:3] + np.array([0.2, 0.0, 0.0])
    down = down / np.linalg.norm(down, axis=1, keepdims=True) + lift * radial
    normals = (down / np.linalg.norm(down, axis=1, keepdims=True)).astype(np.float32)
    storePly(str(root / "sparse" / "0" / "points3D.ply"), pts.astype(np.float32), np.full((pts.shape[0], 3), 128, np.uint8), normals)
    hv = rng.normal(size=(400, 3))
    hv = HEAD_R * hv / np.linalg.norm(hv, axis=1, keepdims=True)
    np.savez(root / "head_reconstruction_data.npz", head_verts=hv, scalp_verts=upper(n_roots, HEAD_R, HEAD_R, 0.3))
    if sdf:
        v, f = HC.uv_sphere(rings=12, segments=16, radius=HEAD_R, centre=(0.0, 0.0, 0.0))
        H.save_sdf(H.scene_sdf_path(str(root)), H.build_sdf(v, f, grid=24, pad=0.1))
    return pts, normals
