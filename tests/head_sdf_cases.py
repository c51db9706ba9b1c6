"""Meshes, grids and point sets of the head distance field's tests (tests/test_head_sdf_cpu.py, tests/test_head_sdf_gpu.py): the
smallest at which the kernels of csrc/hgs_sdf.hip can go wrong.  Every mesh is wound counter-clockwise seen from outside."""
import numpy as np

NEAR = 1e-9          # a node whose reference winding number lies this close to 0.5 has no decided sign
NEAR_SHARE = 1e-3    # at most this share of a case's nodes may be such


def tetrahedron():
    v = np.array([[0.91, 0.13, -0.37], [-0.52, 0.83, -0.29], [-0.41, -0.77, -0.33], [0.07, 0.05, 0.88]])
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    return v, f


def cube(scale=(1.0, 1.0, 1.0)):
    v = np.array([[x, y, z] for z in (-1.0, 1.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)]) * np.asarray(scale)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]])
    return v, f


def uv_sphere(rings=16, segments=16, radius=0.8, centre=(0.03, -0.02, 0.05), open_bottom=False):
    """2*segments cap faces + 2*segments*(rings - 2) others (480 at 16 x 16); open_bottom leaves the south cap out: a "neck"."""
    c = np.asarray(centre)
    v = [c + [0.0, 0.0, radius]]
    for r in range(1, rings):
        th = np.pi * r / rings
        for s in range(segments):
            ph = 2.0 * np.pi * s / segments
            v.append(c + radius * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    v.append(c - [0.0, 0.0, radius])
    south = len(v) - 1
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments        # noqa: E731
    f = [[0, ring(1, s), ring(1, s + 1)] for s in range(segments)]
    for r in range(1, rings - 1):
        for s in range(segments):
            f += [[ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)], [ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)]]
    if not open_bottom:
        f += [[south, ring(rings - 1, s + 1), ring(rings - 1, s)] for s in range(segments)]
    return np.array(v), np.array(f)


def dirty_cube():
    """The cube with face 3 twice, a zero-area face, and a face on a NaN vertex: (verts, faces, dropped, degenerate)."""
    v, f = cube()
    v = np.concatenate([v, [[np.nan, 0.0, 0.0]]])
    f = np.concatenate([f, f[3:4], [[0, 7, 7]], [[0, 1, 8]]])
    return v, f, 1, 1


def counted(n_faces):
    """A 256-face sphere (9 rings x 16) with one face less, as it is, or with one small loose triangle more: an LDS tile's edge."""
    v, f = uv_sphere(rings=9, segments=16)
    assert f.shape[0] == 256
    if n_faces == 255:
        return v, f[:-1]
    if n_faces == 257:
        k = v.shape[0]
        v = np.concatenate([v, [[1.3, 0.1, 0.0], [1.3, 0.2, 0.05], [1.35, 0.12, 0.1]]])
        f = np.concatenate([f, [[k, k + 1, k + 2]]])
    return v, f


def mesh_cases():
    """name -> (verts, faces, grid, pad)."""
    d = dirty_cube()
    return {
        "tetra_g2": (*tetrahedron(), 2, 0.1),
        "tetra_g5": (*tetrahedron(), 5, 0.1),          # 125 nodes: no multiple of 64
        "cube_g5": (*cube(), 5, 0.1),
        "cube_g17": (*cube(), 17, 0.1),
        "flat_cube_g17": (*cube((1.0, 0.6, 0.2)), 17, 0.05),   # a clearly non-cubic grid
        "sphere_g17": (*uv_sphere(), 17, 0.1),
        "open_sphere_g17": (*uv_sphere(open_bottom=True), 17, 0.1),
        "dirty_cube_g5": (d[0], d[1], 5, 0.1),
        "faces_255_g5": (*counted(255), 5, 0.1),
        "faces_256_g5": (*counted(256), 5, 0.1),
        "faces_257_g5": (*counted(257), 5, 0.1),
    }


MESH_NAMES = tuple(mesh_cases())
CLOSED = ("tetra_g2", "tetra_g5", "cube_g5", "cube_g17", "flat_cube_g17", "sphere_g17", "faces_256_g5")


# ---- fields and points of the term ---------------------------------------------------------------------------------------
def ball_field():
    """An analytic field whose grid arithmetic is exact in float32: origin (-1, -0.75, -0.5), h = 1/8, 17 x 13 x 9 nodes, phi the distance
    to a sphere of radius 0.4 about (0.1, -0.05, 0.02).  Not cubic, not symmetric: a swapped axis shows."""
    from utils.head_sdf import HeadSDF
    shape, origin, h = (17, 13, 9), np.array([-1.0, -0.75, -0.5]), 0.125
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(shape[k]) for k in (2, 1, 0)), indexing="ij")
    phi = np.sqrt((x - 0.1) ** 2 + (y + 0.05) ** 2 + (z - 0.02) ** 2) - 0.4
    return HeadSDF(origin, h, shape, phi.astype(np.float32))


def rough_field():
    """A field with nothing exact about it: odd origin and spacing, 7 x 5 x 6 nodes of seeded noise over a slope."""
    from utils.head_sdf import HeadSDF
    rng = np.random.default_rng(11)
    shape, origin, h = (7, 5, 6), np.array([0.137, -2.411, 1.003]), 0.0731
    phi = rng.normal(scale=0.05, size=(shape[2], shape[1], shape[0])) + 0.02 * np.arange(shape[0])[None, None, :] - 0.05
    return HeadSDF(origin, h, shape, phi.astype(np.float32))


FIELDS = {"ball": ball_field, "rough": rough_field}
CENTRE = np.array([0.1, -0.05, 0.02])


def _top(sdf):
    return sdf.origin + (np.array(sdf.shape) - 1) * sdf.spacing


def random_points(sdf, E, seed):
    """E points over the box widened by a fifth: most in range, some out, about a sixth of the ball's inside the sphere."""
    rng = np.random.default_rng(seed)
    lo, hi = sdf.origin, _top(sdf)
    span = hi - lo
    return (lo - 0.1 * span + rng.random((E, 3)) * 1.2 * span).astype(np.float32)


def special_points():
    """On the ball field: nodes, cell faces, t = n - 1 exactly, outside the box, NaN / inf rows, inside by less and by more than a cell."""
    o, h, top = np.array([-1.0, -0.75, -0.5]), 0.125, np.array([1.0, 0.75, 0.5])
    rows = [o + h * np.array([8, 6, 4]), o + h * np.array([9, 5, 4]), o, o + h * np.array([15, 11, 7]),          # nodes
            o + h * np.array([8.0, 5.5, 4.25]), o + h * np.array([9.5, 6.0, 3.75]), o + h * np.array([7.25, 6.5, 4.0]),   # cell faces
            top, [top[0], 0.0, 0.0], [0.0, top[1], 0.0], [0.0, 0.0, top[2]],                                       # t = n - 1: out
            top - [1e-3, 1e-3, 1e-3],                                                                            # the last cell
            [-1.001, 0.0, 0.0], [0.0, 0.9, 0.0], [5.0, 5.0, 5.0], [0.0, 0.0, -0.5001],                             # outside the box
            [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan],
            CENTRE + [0.30, 0.0, 0.0], CENTRE + [0.0, -0.32, 0.0], CENTRE + [0.0, 0.0, 0.34],                      # inside by less than a cell
            CENTRE + [0.1, 0.05, 0.0], CENTRE, CENTRE + [-0.12, 0.08, 0.03],                                      # by more than one
            CENTRE + [0.41, 0.0, 0.0], CENTRE + [0.0, 0.29, 0.29]]                                                # outside, within a margin of 0.05
    return np.array(rows, np.float64).astype(np.float32)


def all_outside(E=130):
    """Points of the ball field's box that the sphere does not reach, margin 0.05 included, and points out of range."""
    rng = np.random.default_rng(3)
    p = random_points(ball_field(), 4 * E, 5)
    far = np.linalg.norm(p.astype(np.float64) - CENTRE, axis=1) > 0.4 + 0.05 + 0.125
    p = p[far][:E]
    assert p.shape[0] == E and rng is not None
    return p


def point_cases():
    """name -> (field name, points f32 [E, 3], margin)."""
    cases = {f"ball_E{E}": ("ball", random_points(ball_field(), E, 100 + E), 0.0) for E in (0, 1, 63, 64, 65, 257)}
    cases["ball_E5000_margin"] = ("ball", random_points(ball_field(), 5000, 7), 0.05)      # several blocks of partial sums
    cases["ball_special"] = ("ball", special_points(), 0.0)
    cases["ball_special_margin"] = ("ball", special_points(), 0.05)
    cases["ball_all_outside"] = ("ball", all_outside(), 0.05)
    cases["rough_E257_margin"] = ("rough", random_points(rough_field(), 257, 9), 0.03)
    cases["rough_E65"] = ("rough", random_points(rough_field(), 65, 10), 0.0)
    return cases


POINT_NAMES = ("ball_E0", "ball_E1", "ball_E63", "ball_E64", "ball_E65", "ball_E257", "ball_E5000_margin", "ball_special",
               "ball_special_margin", "ball_all_outside", "rough_E257_margin", "rough_E65")
