"""Grids, points, centres, the hand-written rays, the gated moments restatement and the quality scene shared by
tests/test_visibility_cpu.py and tests/test_visibility_gpu.py."""
import functools

import numpy as np

from tests import carve_cases as CC
from tests import lift_cases as LC
from tests import visibility_reference as VR

GRIDS = ((1, 1, 1), (2, 2, 2), (5, 4, 3), (17, 9, 6))             # (nx, ny, nz)
DENSITIES = (0.3, 0.9)
NS = (0, 1, 63, 64, 65, 257)
VS = (1, 31, 32, 33, 65)
SKIPS = (0, 1, 3)
MAX_BLOCKED = (0, 2)
ORIGIN, H = np.array([-0.4, 0.25, 1.5]), 0.37                      # (a grid that is neither at zero nor of a round size)


# ---- the equality cases ----------------------------------------------------------------------------------------------------
def random_occ(dims, density, seed=0):
    nx, ny, nz = dims
    return (np.random.default_rng(seed).random((nz, ny, nx)) < density).astype(np.uint8)


def equality_inputs(dims, n=max(NS), v=max(VS), seed=0):
    """(points [n, 3], centres [v, 3]) for the grid `dims` at ORIGIN, H: points over the box and a margin around it, the first ones on
    voxel faces, on the origin and on the far face; centres far outside, close by and inside the box, some sharing a coordinate with a
    point (D_a == 0) and one equal to a point."""
    rng = np.random.default_rng(seed)
    size = np.array(dims, np.float64) * H
    pts = ORIGIN + rng.uniform(-0.1, 1.1, (n, 3)) * size
    special = np.array([ORIGIN, ORIGIN + size, ORIGIN + np.array([H, 0.5 * H, 0.5 * H]), ORIGIN + 0.5 * size,
                        ORIGIN + np.array([size[0], 0.5 * H, 0.5 * H]), [np.nan, ORIGIN[1], ORIGIN[2]]])
    pts[1:1 + len(special)] = special                             # (row 0 stays a random point: N = 1 is a plain one)
    u = rng.normal(size=(v, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    C = ORIGIN + 0.5 * size + u * (np.linalg.norm(size) * rng.choice([0.2, 0.8, 3.0], size=(v, 1)))
    C[0] = pts[0] + np.array([0.0, 0.0, 5.0 * size[2]])           # axis-aligned with point 0
    if v > 2:
        C[1] = pts[4]                                             # the centre of the box: a camera inside, and equal to a point
        C[2, 0] = pts[0, 0]
    return np.ascontiguousarray(pts[:n]), np.ascontiguousarray(C)


@functools.lru_cache(maxsize=None)
def loop_truth(dims, density, skip, max_blocked):
    """(occ, points, centres, bool [257, 65]) of the loop restatement at the largest N and V; a smaller case is a prefix of it (a
    pair's bit depends on nothing but its point, its centre and the grid)."""
    occ = random_occ(dims, density, seed=sum(dims))
    pts, C = equality_inputs(dims)
    return occ, pts, C, VR.visible_loop(pts, C, occ, ORIGIN, H, skip, max_blocked)


# ---- hand-written rays, each with the expected bits ---------------------------------------------------------------------------
def _occ(dims, *voxels, fill=0):
    nx, ny, nz = dims
    occ = np.full((nz, ny, nx), fill, np.uint8)
    for x, y, z in voxels:
        occ[z, y, x] = 1 - fill
    return occ


def hand_cases():
    """[(name, points, centres, occ, origin, h, skip, max_blocked, want bool [N, V])]; origin 0 and h = 1 unless the name says so:
    every crossing time is exact."""
    inf, nan = float("inf"), float("nan")
    o0 = np.zeros(3)
    row, cube = (8, 1, 1), (4, 4, 4)
    mid = [0.5, 0.5, 0.5]
    far = [[20.0, 0.5, 0.5]]
    cases = [
        # t = 1 belongs to voxel 1: towards -x the ray enters voxel 0 at once, towards +x voxel 2
        ("a point on a voxel face", [[1.0, 0.5, 0.5]], [[-5.0, 0.5, 0.5], [9.0, 0.5, 0.5]], _occ(cube, (0, 0, 0)), o0, 1.0, 0, 0, [[0, 1]]),
        ("the same with the other neighbour occupied", [[1.0, 0.5, 0.5]], [[-5.0, 0.5, 0.5], [9.0, 0.5, 0.5]], _occ(cube, (2, 0, 0)), o0, 1.0, 0, 0,
         [[1, 0]]),
        # the origin is inside (voxel 0): every tmax towards (-1, -1, -1) is -0, x wins and leaves the grid
        ("a point on the origin", [[0.0, 0.0, 0.0]], [[-1.0, -1.0, -1.0], [5.0, 0.0, 0.0]], _occ(cube, fill=1), o0, 1.0, 0, 0, [[1, 0]]),
        ("a point on the far face is outside", [[4.0, 0.5, 0.5], [0.5, 4.0, 0.5], [0.5, 0.5, 4.0]], [[-5.0, 0.5, 0.5]], _occ(cube, fill=1), o0, 1.0,
         0, 0, [[1], [1], [1]]),
        ("axis-aligned rays", [[1.5, 1.5, 1.5]], [[1.5, 1.5, 9.0], [1.5, -9.0, 1.5], [9.0, 1.5, 1.5]], _occ(cube, (1, 1, 3), (1, 0, 1)), o0, 1.0, 1, 0,
         [[0, 1, 1]]),
        # D = (3, 3, 3) from a voxel centre: the three tmax are equal at every corner, and x, then y, then z is taken
        ("the diagonal, the x neighbour occupied", [mid], [[3.5, 3.5, 3.5]], _occ(cube, (1, 0, 0)), o0, 1.0, 0, 0, [[0]]),
        ("the diagonal, the y neighbour occupied", [mid], [[3.5, 3.5, 3.5]], _occ(cube, (0, 1, 0)), o0, 1.0, 0, 0, [[1]]),
        ("the diagonal, the z neighbour occupied", [mid], [[3.5, 3.5, 3.5]], _occ(cube, (0, 0, 1)), o0, 1.0, 0, 0, [[1]]),
        ("the diagonal, the voxel after x and y", [mid], [[3.5, 3.5, 3.5]], _occ(cube, (1, 1, 0)), o0, 1.0, 0, 0, [[0]]),
        # the camera sits in voxel 3: that voxel is entered and tested, the one behind it is not
        ("a camera inside the grid, occupied beyond it", [mid], [[3.5, 0.5, 0.5]], _occ(row, (4, 0, 0), (7, 0, 0)), o0, 1.0, 1, 0, [[1]]),
        ("a camera inside the grid, its own voxel occupied", [mid], [[3.5, 0.5, 0.5]], _occ(row, (3, 0, 0)), o0, 1.0, 1, 0, [[0]]),
        ("a camera in the point's own voxel", [[0.25, 0.5, 0.5]], [[0.75, 0.625, 0.5]], _occ(cube, fill=1), o0, 1.0, 0, 0, [[1]]),
        ("a point equal to the camera", [[1.25, 2.5, 0.75]], [[1.25, 2.5, 0.75]], _occ(cube, fill=1), o0, 1.0, 0, 0, [[1]]),
        ("NaN, infinite and 1e300 points", [[nan, 0.5, 0.5], [0.5, nan, 0.5], [0.5, 0.5, nan], [inf, 0.5, 0.5], [0.5, -inf, 0.5], [0.5, 0.5, inf],
                                            [1e300, 0.5, 0.5], [0.5, -1e300, 0.5], [1e300, 1e300, 1e300]],
         [[20.0, 0.5, 0.5], [0.5, 0.5, 0.5]], _occ(cube, fill=1), o0, 1.0, 0, 0, [[1, 1]] * 9),
        ("an occupied start voxel", [mid], far, _occ(row, (0, 0, 0)), o0, 1.0, 0, 0, [[1]]),
        ("a blocker at Chebyshev distance skip", [mid], far, _occ(row, (2, 0, 0)), o0, 1.0, 2, 0, [[1]]),
        ("a blocker at Chebyshev distance skip + 1", [mid], far, _occ(row, (3, 0, 0)), o0, 1.0, 2, 0, [[0]]),
        ("max_blocked blockers", [mid], far, _occ(row, (1, 0, 0), (4, 0, 0)), o0, 1.0, 0, 2, [[1]]),
        ("max_blocked + 1 blockers", [mid], far, _occ(row, (1, 0, 0), (4, 0, 0), (6, 0, 0)), o0, 1.0, 0, 2, [[0]]),
        # (a grid away from zero with h = 0.5: the same ray as "skip + 1", in halves, which are exact too)
        ("origin (-1, 2, 3), h = 0.5", [[-0.75, 2.25, 3.25]], [[9.0, 2.25, 3.25]], _occ(row, (3, 0, 0)), np.array([-1.0, 2.0, 3.0]), 0.5, 2, 0, [[0]]),
    ]
    return [(name, np.array(p, np.float64), np.array(c, np.float64), occ, np.asarray(o, np.float64), h, s, m, np.array(w, bool))
            for name, p, c, occ, o, h, s, m, w in cases]


# ---- the gated moments, restated ----------------------------------------------------------------------------------------------
def gated_moments_loop(points, views, masks, orients, confs, tab, visible, prev=None, s2=0.0, min_conf=1):
    """utils/lift.py's gated moments through lift_cases.moments_loop: point by point, over the views whose bit is set, in their order.
    A view that is not used adds nothing to a sum, so leaving it out of the loop is the gate.  visible: bool [N, V]."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    N = pts.shape[0]
    M, wsum, count = np.zeros((N, 6), np.float64), np.zeros(N, np.float64), np.zeros(N, np.int32)
    for i in range(N):
        ks = [k for k in range(len(views)) if visible[i, k]]
        if ks:
            m, w, c = LC.moments_loop(pts[i:i + 1], [views[k] for k in ks], [masks[k] for k in ks], [orients[k] for k in ks],
                                      [confs[k] for k in ks], tab, None if prev is None else prev[i:i + 1], s2, min_conf)
            M[i], wsum[i], count[i] = m[0], w[0], c[0]
    return M, wsum, count


def random_visible(N, V, seed=0, share=0.6):
    """bool [N, V] with about `share` set; the first row all set, the second none."""
    vis = np.random.default_rng(seed).random((N, V)) < share
    vis[:1] = True
    vis[1:2] = False
    return vis


# ---- the quality scene --------------------------------------------------------------------------------------------------------
Q_VIEWS, Q_SIZE, Q_F, Q_RING, Q_GRID, Q_HALF, Q_RADIUS = 12, 64, 70.0, 3.0, 24, 0.8, 0.6
Q_AXIS = np.array([0.2, 0.3, 1.0])


def quality_truth(q):
    t = np.cross(Q_AXIS, q)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def quality_scene():
    """dict(views, centres, occ, origin, h, points [792, 3], truth, orient uint8 [V, N], chord [N, V]): 12 ring views of a 24^3 grid
    over [-0.8, 0.8]^3 whose voxels within 0.6 of the origin are occupied; the points are the shell's centres, the hair runs along
    cross((0.2, 0.3, 1), q), and every view samples, for a point, the image angle of the hair at the FIRST hit of the point's ray with
    the sphere of the point's own radius: a far-side view reports the near side's hair.  chord: the distance from that hit to the
    point."""
    from utils import carve
    from utils.carve import View
    from utils.visibility import camera_centres
    views = []
    for k in range(Q_VIEWS):
        a = 2.0 * np.pi * k / Q_VIEWS + 0.2
        R, t = CC.look_at((Q_RING * np.cos(a), Q_RING * np.sin(a), (-1.0, 0.4, 1.4, -0.3)[k % 4]))
        views.append(View(R=R, t=t, fx=Q_F, fy=Q_F, cx=Q_SIZE / 2, cy=Q_SIZE / 2, W=Q_SIZE, H=Q_SIZE, name=f"quality_{k}.png"))
    origin, h, dims = np.full(3, -Q_HALF), 2.0 * Q_HALF / Q_GRID, (Q_GRID,) * 3
    xs, ys, zs = carve.centres(origin, h, dims)
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    occ = (np.sqrt(X * X + Y * Y + Z * Z) <= Q_RADIUS).astype(np.uint8)
    shell = carve.shell_numpy(occ) != 0
    pts = np.ascontiguousarray(np.stack([X[shell], Y[shell], Z[shell]], axis=1))
    C = camera_centres(views)
    orient = np.zeros((Q_VIEWS, pts.shape[0]), np.uint8)
    chord = np.zeros((pts.shape[0], Q_VIEWS))
    for k, v in enumerate(views):
        d = pts - C[k]                                            # |C + s d| = |q|: s = 1 is the point, the other root the other hit
        A, B = (d * d).sum(axis=1), (d * C[k]).sum(axis=1)
        s = np.minimum(1.0, -2.0 * B / A - 1.0)                   # (the roots sum to -2B/A)
        x = C[k] + s[:, None] * d
        orient[k], inside = LC.image_angle_bytes([v], x, quality_truth(x))
        assert inside.all()
        chord[:, k] = np.linalg.norm(x - pts, axis=1)
    return dict(views=views, centres=C, occ=occ, origin=origin, h=h, points=pts, truth=quality_truth(pts), orient=orient, chord=chord)


def quality_lift(scene, visible=None, rounds=0):
    """The direction [N, 3] after `rounds` re-weighted rounds of the scene's samples (confidence 255), gated by the words or not."""
    from utils import lift
    used = np.ones(scene["orient"].shape, bool)
    conf = np.full(scene["orient"].shape, 255, np.uint8)
    s2, prev = lift.sin2(10.0), None
    for _ in range(rounds + 1):
        M, _, count = lift.moments_from_samples(scene["points"], scene["views"], used, scene["orient"], conf, prev, s2, visible=visible)
        prev, _ = lift.solve_numpy(M, count)
    return prev
