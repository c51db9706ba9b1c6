"""Gaussians by CLASS for the float64 check of the rasterizer's per-Gaussian backward (preprocess_bwd_kernel,
csrc/hgs_preprocess.hip): every class holds N rows that share the property it is listed for -- a branch of the chain
conic -> cov2D -> T, J -> view-space mean -> dL_dmeans3D, dL_dcov3D -> dL_dscales, dL_drotations, colour -> SH -- and are
random within it.  Rows are built in float64 in the VIEW space of one axis-aligned camera (64 x 48, fovx 60 degrees, eye
(0, 0, -1.2): world = view - (0, 0, 1.2f), the view matrix holds 0, 1 and 1.2f only) and rounded ONCE to float32.  numpy only.

The classes are concatenated into one scene, `hard_gaussians`, with opacities in [0.01, 0.04] (nothing saturates), in four
input forms: `sh0` (sh_degree 0, M = 1: the DC_ONLY instantiation), `sh3` (sh_degree 3, M = 16), `colors_precomp`,
`cov3D_precomp`.  tests/gaussian_reference.py grades them row by row; tests/test_gaussians_f64_cpu.py asserts what the classes
promise.
"""
import functools
import math

import numpy as np

from tests import scenes

W, H, FOVX_DEG = 64, 48, 60.0
EYE = (0.0, 0.0, -1.2)
N = 64                                   # rows per class
BG = (0.2, 0.1, 0.3)
FORMS = ("sh0", "sh3", "colors_precomp", "cov3D_precomp")
FAR_SHIFT = (100.0, -50.0, 25.0)
# Classes whose rows sit ON the float32 grid of the base camera (a pair of neighbouring view depths, a ratio within ulps of
# the clamp): they exist at the base camera only.
GRID_CLASSES = ("clamp_edge", "near_cut")
CLASSES = ("plain", "clamp_x", "clamp_y", "clamp_xy", "clamp_edge", "near", "near_cut", "needle_side", "needle_diag",
           "needle_endon", "near_needle", "tiny", "qnorm", "sh_clamped")
SH_C0 = float(np.float32(0.28209479177387814))
SH_C1 = float(np.float32(0.4886025119029199))
SH_C2 = [float(np.float32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                                         0.5462742152960396)]
SH_C3 = [float(np.float32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                                         -0.4570457994644658, 1.445305721320277, -0.5900435899266435)]


def camera(far_origin=False):
    """The camera, with the two tangents rounded to float32 so that the fp32 and the float64 statement receive the SAME numbers
    (the C ABI takes them as float)."""
    shift = np.asarray(FAR_SHIFT if far_origin else (0.0, 0.0, 0.0))
    cam = scenes.make_camera(eye=np.asarray(EYE) + shift, target=shift, W=W, H=H, fovx_deg=FOVX_DEG)
    cam["tanfovx"], cam["tanfovy"] = float(np.float32(cam["tanfovx"])), float(np.float32(cam["tanfovy"]))
    return cam


def sh_rest(d, sh):
    """Sum of the SH terms of order >= 1 (CR/forward.cu:20-71) for unit directions d [n, 3] and coefficients sh [n, 16, 3], in
    float64: what the DC coefficient has to balance."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b = [-SH_C1 * y, SH_C1 * z, -SH_C1 * x, SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz,
         SH_C2[4] * (xx - yy), SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
         SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
         SH_C3[6] * x * (xx - 3.0 * yy)]
    return sum(bk[:, None] * sh[:, k + 1, :].astype(np.float64) for k, bk in enumerate(b))


def _unit_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _quat_x_to(d):
    """Unit quaternion (r, x, y, z) that turns x_hat into the unit vector d (d.x >= 0 here: far from the half turn)."""
    q = np.stack([1.0 + d[:, 0], np.zeros(len(d)), -d[:, 2], d[:, 1]], 1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), size))


def _on_screen(rng, n, tz, tanx, tany):
    """View-space x, y at depth tz whose projection lies 0.05 .. 0.3 px (either sign, both axes) off a pixel centre at least 4
    px inside the image: a footprint of sigma = sqrt(0.3) px (the low-pass alone) still reaches alpha >= 1 / 255 at opacity
    0.01, and no footprint is symmetric about a pixel."""
    off = lambda: rng.uniform(0.05, 0.3, n) * rng.choice([-1.0, 1.0], n)   # noqa: E731
    u, v = rng.integers(4, W - 4, n) + off(), rng.integers(4, H - 4, n) + off()
    return ((2.0 * u + 1.0) / W - 1.0) * tanx * tz, ((2.0 * v + 1.0) / H - 1.0) * tany * tz


def _needle_scales(L):
    return np.stack([L, np.full_like(L, 1e-4), np.full_like(L, 1e-4)], 1)


def _positive_x(d):
    return d * np.where(d[:, :1] < 0, -1.0, 1.0)


def _class_rows(name, rng, cam):
    """(view-space position [N, 3], scales [N, 3], quaternion [N, 4]) of one class, float64."""
    tanx, tany = cam["tanfovx"], cam["tanfovy"]
    tz = rng.uniform(0.8, 1.6, N)
    scales = _log_uniform(rng, 0.02, 0.1, (N, 3))
    q = _unit_quat(rng, N)
    if name in ("plain", "sh_clamped"):
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
    elif name in ("clamp_x", "clamp_y", "clamp_xy"):
        # off screen by 0.32 .. 0.45 half-widths; scales 0.2 .. 0.5 so that every row's tail still reaches the screen
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        far = lambda tan: rng.uniform(1.32, 1.45, N) * rng.choice([-1.0, 1.0], N) * tan * tz   # noqa: E731
        if name != "clamp_y":
            tx = far(tanx)
        if name != "clamp_x":
            ty = far(tany)
        scales = rng.uniform(0.2, 0.5, (N, 3))
    elif name == "near":
        tz = rng.uniform(0.2005, 0.23, N)
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        scales = _log_uniform(rng, 0.005, 0.03, (N, 3))
    elif name in ("needle_side", "needle_diag"):
        tz = rng.uniform(0.9, 1.5, N)
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        if name == "needle_side":      # in the image plane, within 15 degrees of a screen axis
            phi = np.radians(rng.uniform(-15.0, 15.0, N) + rng.choice([0.0, 90.0], N))
            L = rng.uniform(0.02, 0.08, N)
        else:                          # within 5 degrees of a screen diagonal: cov2D has a ~ c ~ |b|, a c - b^2 cancels
            phi = np.radians(rng.uniform(-5.0, 5.0, N) + rng.choice([-45.0, 45.0], N))
            L = rng.uniform(0.02, 0.05, N)
        d = _positive_x(np.stack([np.cos(phi), np.sin(phi), np.zeros(N)], 1))
        scales, q = _needle_scales(L), _quat_x_to(d)
    elif name == "needle_endon":       # along the ray through the mean, tilted by at most 3 degrees
        tz = rng.uniform(0.9, 1.5, N)
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        ray = np.stack([tx, ty, tz], 1)
        ray /= np.linalg.norm(ray, axis=1, keepdims=True)
        side = np.cross(ray, rng.normal(size=(N, 3)))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        d = ray + np.tan(np.radians(rng.uniform(0.0, 3.0, N)))[:, None] * side
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        scales, q = _needle_scales(rng.uniform(0.02, 0.08, N)), _quat_x_to(d)
    elif name == "near_needle":
        tz = rng.uniform(0.2005, 0.23, N)
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        d = rng.normal(size=(N, 3))
        d = _positive_x(d / np.linalg.norm(d, axis=1, keepdims=True))
        scales, q = _needle_scales(rng.uniform(0.003, 0.01, N)), _quat_x_to(d)
    elif name == "tiny":               # the floor of the strand forward on all three axes: cov2D is the low-pass alone
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        scales = np.full((N, 3), 1e-7)
    elif name == "qnorm":              # used unnormalised (CR/forward.cu:127): |q| in [0.3, 3] scales the covariance by |q|^4
        tx, ty = _on_screen(rng, N, tz, tanx, tany)
        scales = _log_uniform(rng, 0.01, 0.04, (N, 3))
        q = q * _log_uniform(rng, 0.3, 3.0, (N, 1))
    elif name in GRID_CLASSES:
        tx, ty = _on_screen(rng, N, tz, tanx, tany)    # (x and z are set on the float32 grid by _snap_to_grid)
        scales = _log_uniform(rng, 0.005, 0.03, (N, 3)) if name == "near_cut" else rng.uniform(0.2, 0.5, (N, 3))
    else:
        raise KeyError(name)
    return np.stack([tx, ty, tz], 1), scales, q


def near_cut_depths(cam):
    """(world z of the culled row, world z of the kept row, their float32 view depths): the two NEIGHBOURING float32 world
    depths whose fp32 view depth fl(z + 1.2f) lies on either side of the `<= 0.2f` cut (CR/auxiliary.h:154).  z is a multiple
    of 2^-23 below -1 and of 2^-24 above, 1.2f one of 2^-23, so the sum is exact and a multiple of 2^-24; 0.2f = 13421773 x
    2^-26 is not, and nextafter(0.2f, 1) is not either: the pair nearest to the cut that this camera can produce is taken."""
    tz = np.float32(cam["viewmatrix"][3, 2])
    z = np.float32(np.float64(np.float32(0.2)) - np.float64(tz))
    while np.float32(z + tz) <= np.float32(0.2):
        z = np.nextafter(z, np.float32(1.0))
    while np.float32(np.nextafter(z, np.float32(-2.0)) + tz) > np.float32(0.2):
        z = np.nextafter(z, np.float32(-2.0))
    lo = np.nextafter(z, np.float32(-2.0))
    return lo, z, np.float32(lo + tz), np.float32(z + tz)


def _snap_to_grid(name, rng, cam, xyz32):
    """The two classes that live on the float32 grid (base camera: world x = view x, view z = fl(world z + 1.2f))."""
    tz32 = np.float32(cam["viewmatrix"][3, 2])
    if name == "near_cut":             # rows 2k (culled) and 2k + 1 (graded) differ in the last bit of world z only
        lo, hi, _, _ = near_cut_depths(cam)
        tz_view = float(hi) + float(tz32)
        even = xyz32[0::2].copy()
        even[:, 0] *= np.float32(tz_view) / (even[:, 2] + tz32)    # keep the projection on the screen at the new depth
        even[:, 1] *= np.float32(tz_view) / (even[:, 2] + tz32)
        xyz32[0::2], xyz32[1::2] = even, even
        xyz32[0::2, 2], xyz32[1::2, 2] = lo, hi
    else:                              # clamp_edge: fp32 t.x / t.z within 2 ulp of +-fl(1.3f tan_fovx), on both sides
        lim = np.float32(1.3) * np.float32(cam["tanfovx"])
        tz = xyz32[:, 2] + tz32
        x = (lim * tz).astype(np.float32)
        k = np.arange(len(x)) % 5 - 2
        for step in (1, 2):
            x = np.where(k >= step, np.nextafter(x, np.float32(np.inf)), np.where(k <= -step, np.nextafter(x, np.float32(0)), x))
        xyz32[:, 0] = x * rng.choice(np.float32([-1.0, 1.0]), len(x))
    return xyz32


@functools.lru_cache(maxsize=None)
def _rows(far_origin, scale_modifier):
    """Every class, concatenated: the float32 arrays of the scene and {class: row indices}."""
    cam = camera(far_origin)
    names = [c for c in CLASSES if not (far_origin and c in GRID_CLASSES)]
    t_view = cam["viewmatrix"][3, :3].astype(np.float64)           # view = world + t_view (the rotation is the identity)
    assert np.array_equal(cam["viewmatrix"][:3, :3], np.eye(3, dtype=np.float32))
    xyz, scales, quats, classes = [], [], [], {}
    for ci, name in enumerate(names):
        rng = np.random.default_rng(1000 + CLASSES.index(name))
        pv, sc, q = _class_rows(name, rng, cam)
        x32 = (pv - t_view).astype(np.float32)
        if name in GRID_CLASSES:
            x32 = _snap_to_grid(name, rng, cam, x32)
        xyz.append(x32)
        scales.append((sc / scale_modifier).astype(np.float32))    # the SAME scene at every modifier
        quats.append(q.astype(np.float32))
        classes[name] = np.arange(ci * N, (ci + 1) * N)
    xyz, scales, quats = np.concatenate(xyz), np.concatenate(scales), np.concatenate(quats)
    P = xyz.shape[0]
    rng = np.random.default_rng(77)
    opac = rng.uniform(0.01, 0.04, P).astype(np.float32)
    shs = (rng.normal(size=(P, 16, 3)) * 0.15).astype(np.float32)
    shs[:, 0, :] += np.float32(0.8)
    colors = rng.uniform(-0.5, 1.0, (P, 3)).astype(np.float32)
    # sh_clamped: one or two channels with result + 0.5 below 0 by 1.2e-4 .. 0.3, one 1.2e-4 .. 9e-4 above 0 (the margins of the
    # class, 1e-4 and [1e-4, 1e-3], with room for the rounding of the DC coefficient and of the fp32 evaluation, ~1e-6)
    r = classes["sh_clamped"]
    target = np.empty((N, 3))
    two = rng.random(N) < 0.5
    target[:, 0] = -_log_uniform(rng, 1.2e-4, 0.3, N)
    target[:, 1] = rng.uniform(1.2e-4, 9e-4, N)
    target[:, 2] = np.where(two, -_log_uniform(rng, 1.2e-4, 0.3, N), rng.uniform(0.2, 0.9, N))
    target = np.take_along_axis(target, np.argsort(rng.random((N, 3)), axis=1), axis=1)   # which channel is which: shuffled
    d = xyz[r].astype(np.float64) - cam["campos"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shs3 = shs.copy()
    shs3[r, 0, :] = ((target - 0.5 - sh_rest(d, shs[r])) / SH_C0).astype(np.float32)
    shs0 = shs[:, :1, :].copy()
    shs0[r, 0, :] = ((target - 0.5) / SH_C0).astype(np.float32)
    L = scenes.quat_to_rotmat(quats.astype(np.float64)) * scales.astype(np.float64)[:, None, :]
    cov = L @ np.transpose(L, (0, 2, 1))
    cov6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1).astype(np.float32)
    for a in (xyz, scales, quats, opac, shs0, shs3, colors, cov6):
        a.setflags(write=False)
    return dict(means3D=xyz, scales=scales, rotations=quats, opacities=opac, shs0=shs0, shs3=shs3, colors=colors, cov6=cov6,
                classes=classes, sh_target=target)


def hard_scene(form="sh3", scale_modifier=1.0, far_origin=False, rows=None):
    """The scene `hard_gaussians` in one input form (FORMS); `scale_modifier`: the whole scene again at that modifier (the
    stored scales are divided by it; a precomputed covariance ignores it, as in the reference); `far_origin`: world and camera
    both shifted by FAR_SHIFT (without GRID_CLASSES); `rows`: indices of a subset.  Extra keys: `classes` {name: row indices
    into the returned arrays}, `form`."""
    assert form in FORMS
    scale_modifier = float(np.float32(scale_modifier))
    base = _rows(bool(far_origin), scale_modifier)
    P = base["means3D"].shape[0]
    keep = np.arange(P) if rows is None else np.asarray(rows, np.int64)
    take = lambda a: np.ascontiguousarray(a[keep])   # noqa: E731
    s = dict(camera(far_origin))
    s.update(means3D=take(base["means3D"]), opacities=take(base["opacities"]), bg=np.asarray(BG, np.float32),
             sh_degree=0, scale_modifier=scale_modifier, shs=None, colors_precomp=None, scales=None, rotations=None,
             cov3D_precomp=None, form=form)
    if form == "colors_precomp":
        s["colors_precomp"] = take(base["colors"])
    elif form == "sh0":
        s["shs"] = take(base["shs0"])
    else:
        s["shs"], s["sh_degree"] = take(base["shs3"]), 3
    if form == "cov3D_precomp":
        s["cov3D_precomp"] = take(base["cov6"])
    else:
        s["scales"], s["rotations"] = take(base["scales"]), take(base["rotations"])
    pos = {int(r): i for i, r in enumerate(keep)}
    s["classes"] = {c: np.asarray([pos[int(r)] for r in idx if int(r) in pos], np.int64) for c, idx in base["classes"].items()}
    return s


def _rotmat_to_quat(R):
    """(r, x, y, z) unit quaternions of rotation matrices [n, 3, 3]: the eigenvector of the largest eigenvalue of the symmetric
    4 x 4 form of each (no branch on the trace)."""
    K = np.zeros((R.shape[0], 4, 4))
    K[:, 0, 0] = R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2]
    K[:, 1, 0], K[:, 1, 1] = R[:, 0, 1] + R[:, 1, 0], R[:, 1, 1] - R[:, 0, 0] - R[:, 2, 2]
    K[:, 2, 0], K[:, 2, 1], K[:, 2, 2] = R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1], R[:, 2, 2] - R[:, 0, 0] - R[:, 1, 1]
    K[:, 3, 0], K[:, 3, 1], K[:, 3, 2] = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    K[:, 3, 3] = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    _, vecs = np.linalg.eigh(K / 3.0)                      # (reads the lower triangle; eigenvalues ascending)
    q = vecs[:, [3, 0, 1, 2], 3]
    assert np.abs(scenes.quat_to_rotmat(q) - R).max() < 1e-6     # (a camera's float32 rotation is orthogonal to ~1e-7)
    return q


def rows_in_camera(world_view_transform, tanfovx, tanfovy):
    """(world xyz, scales, quaternions), float32, of the concatenation placed in ANOTHER camera's view space: the rows keep
    their view depth and their position relative to that camera's frustum (x / z and y / z scale with the tangents, so a row
    beyond 1.3 tan stays beyond it), their axes turn with the camera.  For models that hold raw parameters (the fused
    iterations of tests/test_gpu_train.py); `world_view_transform` is the transposed 4 x 4 matrix of a Camera."""
    base, cam = _rows(False, 1.0), camera()
    wvt = np.asarray(world_view_transform, np.float64)
    pv = base["means3D"].astype(np.float64) + cam["viewmatrix"][3, :3].astype(np.float64)
    pv[:, 0] *= tanfovx / cam["tanfovx"]
    pv[:, 1] *= tanfovy / cam["tanfovy"]
    world = (np.concatenate([pv, np.ones((len(pv), 1))], 1) @ np.linalg.inv(wvt))[:, :3]
    q = base["rotations"].astype(np.float64)
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    q_world = _rotmat_to_quat(wvt[:3, :3] @ scenes.quat_to_rotmat(q / norm)) * norm
    return world.astype(np.float32), base["scales"].copy(), q_world.astype(np.float32)


def spread_rows(n, P=None):
    """n rows of the concatenation, evenly spread over it (every class is met once n >= the number of classes)."""
    P = len(CLASSES) * N if P is None else P
    return (np.arange(n, dtype=np.int64) * P) // n


def smooth_dpix():
    """dL_dpix: a smooth ramp without a symmetry (no noise), so that dL_dmeans2D and dL_dconic of a footprint do not cancel."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((3, H, W))
    for c, (a, bx, by, ph) in enumerate(((0.6, 0.5, -0.35, 0.3), (-0.4, 0.3, 0.45, 1.1), (0.3, -0.55, 0.25, 2.0))):
        out[c] = a + bx * x / W + by * y / H + 0.2 * np.sin(0.11 * x + 0.07 * y + ph)
    return out.astype(np.float32)
