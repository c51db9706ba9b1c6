"""The head mesh of a capture as a signed distance field on a regular grid, and the penetration term that samples it at the strand
joints: from Stage II on the strands are free polylines, the head is not rendered and the hair on top hides a joint that has sunk below
the skin, so no image term sees it.  head_sdf.py is the scene driver and writes head_sdf.npz; train.py --lambda_head loads it; the
reference has no such term (loss/losses.py).

The contract (this module's numpy paths, csrc/hgs_sdf.hip and the loop restatement in tests/head_sdf_reference.py state the same
thing).  The field is float64 with one rounding per operation, in exactly the order written; the term is float32 in the same way (the
kernel file is built with -ffp-contract=off).  dot(u, v) = (u0*v0 + u1*v1) + u2*v2 throughout.

Mesh.  utils.scalp.check_mesh validates (verts, faces).  A face with a vertex that is not finite is dropped and counted (`dropped`).
A face whose cross product n = (v1 - v0) x (v2 - v0) has dot(n, n) not finite or not > 0 -- zero area: the only faces for which
the region form below can leave a distance that is not finite -- is skipped and counted (`degenerate`), once, not per node.  The
kernel and the numpy path moreover let a squared distance that is not finite lose every comparison.  No usable face: ValueError.

Box.  lo, hi: the bounding box of the finite vertices; L = max(hi - lo); m = pad*L; origin = lo - m; top = hi + m; side = top - origin;
h = max(side) / (grid - 1); n_axis = ceil(side_axis / h) + 1 (not cubic in general).  2 <= grid <= 512, pad finite and >= 0; h must come
out finite and > 0.  Node (ix, iy, iz) lies at p = origin + index*h; phi is stored [nz, ny, nx], float32.

Magnitude.  Per (node p, face): a = v0 - p, b = v1 - p, c = v2 - p (shared with the sign below); ap = -a, bp = -b, cp = -c;
e1 = v1 - v0, e2 = v2 - v0;
    d1 = dot(e1, ap), d2 = dot(e2, ap), d3 = dot(e1, bp), d4 = dot(e2, bp), d5 = dot(e1, cp), d6 = dot(e2, cp)
    vc = d1*d4 - d3*d2,  vb = d5*d2 - d1*d6,  va = d3*d6 - d5*d4
the first region that applies gives q, the vector from the closest point to p:
    d1 <= 0 and d2 <= 0                              vertex v0     q = ap
    d3 >= 0 and d4 <= d3                             vertex v1     q = bp
    vc <= 0 and d1 >= 0 and d3 <= 0                  edge v0 v1    v = d1/(d1 - d3),                        q = ap - v*e1
    d6 >= 0 and d5 <= d6                             vertex v2     q = cp
    vb <= 0 and d2 >= 0 and d6 <= 0                  edge v0 v2    w = d2/(d2 - d6),                        q = ap - w*e2
    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0        edge v1 v2    w = (d4 - d3)/((d4 - d3) + (d5 - d6)),   q = bp - w*(v2 - v1)
    otherwise                                        interior      s = 1/((va + vb) + vc), v = vb*s, w = vc*s,  q = ap - (e1*v + e2*w)
dist2 = dot(q, q); the node keeps the minimum over the faces (a comparison dist2 < best from best = +inf) and takes one sqrt at the end.
A minimum does not depend on the faces' order or on how the work is split: the kernel and the numpy path give equal bits in |phi|.

Sign.  The generalized winding number: head meshes are open at the neck and have inner cavities, and it degrades gracefully there.
    la = sqrt(dot(a, a)), lb, lc likewise
    det = (a0*(b1*c2 - b2*c1) + a1*(b2*c0 - b0*c2)) + a2*(b0*c1 - b1*c0)
    den = (((la*lb)*lc + dot(a, b)*lc) + dot(b, c)*la) + dot(c, a)*lb
    S += 2*atan2(det, den)   over the faces in order;   w = S / (4 pi)   (4 pi = 12.566370614359172)
A node is inside iff w > 0.5.  This sum depends on the device's atan2 (and would on its order): it is compared by decision, not by bits.

Stored value.  phi = float32(sqrt(best)), negated where inside; a zero is stored as +0.

Term.  sample(points, sdf, margin), float32 operation by operation; o = float32(origin), k = float32(1/h) (the division in float64):
    t = (p - o)*k per axis;   in range  iff  every t is finite and 0 <= t < n_axis - 1;   i = floor(t), f = t - i
    lerp(u, v, f) = u + f*(v - u);   c_xyz = phi[iz + z, iy + y, ix + x]
    c00 = lerp(c000, c100, fx), c10 = lerp(c010, c110, fx), c01 = lerp(c001, c101, fx), c11 = lerp(c011, c111, fx)
    c0 = lerp(c00, c10, fy), c1 = lerp(c01, c11, fy),   d = lerp(c0, c1, fz)
    gx = lerp(lerp(c100 - c000, c110 - c010, fy), lerp(c101 - c001, c111 - c011, fy), fz)*k
    gy = lerp(lerp(c010 - c000, c110 - c100, fx), lerp(c011 - c001, c111 - c101, fx), fz)*k
    gz = lerp(lerp(c001 - c000, c101 - c100, fx), lerp(c011 - c010, c111 - c110, fx), fy)*k
    r = margin - d;   pen = r*r and g = (-2*r)*(gx, gy, gz) where in range and r > 0, else both 0
Points out of range count as outside the head: the box's pad makes that true.  L = float32(sum of pen in float64 / E) over ALL E rows,
so a penetrating minority does not rescale the gradient; L = 0 for E = 0.  dL/dp = g*(upstream/float32(E)): one float32 division, one
multiplication.

Known limits.  Only joints are tested: a long segment can still cut a corner.  The field is only as good as the mesh's alignment to the
cameras.  Near the neck opening the winding number fades instead of switching.  The build is the plain O(nodes x faces) form: the
numpy path is for small grids and the tests.

device=None: numpy.  device="cuda": the kernels.  The caller chooses; neither falls back to the other (utils/carve.py's convention)."""
import math
import os

import numpy as np

from utils.scalp import check_mesh
from utils.views import is_cuda

FILE = "head_sdf.npz"
KEYS = ("origin", "spacing", "shape", "phi", "mesh_faces", "mesh_verts")
MIN_GRID, MAX_GRID = 2, 512
FOUR_PI = 12.566370614359172
_PAIRS = 1 << 19                # (node, face) pairs per numpy pass


class HeadSDF:
    """origin f64 [3], spacing f64, shape (nx, ny, nz), phi float32 [nz, ny, nx]; mesh_faces / mesh_verts: the counts of the mesh it
    was built from (the report's).  The device copies of the field are cached on the object."""

    def __init__(self, origin, spacing, shape, phi, mesh_faces=0, mesh_verts=0):
        self.origin = np.ascontiguousarray(np.asarray(origin, np.float64).reshape(3))
        self.spacing = float(spacing)
        self.shape = tuple(int(n) for n in shape)
        self.phi = np.ascontiguousarray(phi, dtype=np.float32)
        self.mesh_faces, self.mesh_verts = int(mesh_faces), int(mesh_verts)
        nx, ny, nz = self.shape
        if len(self.shape) != 3 or min(self.shape) < 1 or max(self.shape) > 1024 or self.phi.shape != (nz, ny, nx):
            raise ValueError(f"a field of shape {self.phi.shape} for a grid of {self.shape} nodes ([nz, ny, nx], 1 to 1024 an axis)")
        if not (math.isfinite(self.spacing) and self.spacing > 0.0 and np.isfinite(self.origin).all()):
            raise ValueError(f"origin {self.origin.tolist()} and spacing {self.spacing}: finite, the spacing > 0")
        self.origin32 = self.origin.astype(np.float32)
        self.inv_h32 = np.float32(1.0 / self.spacing)
        if not (np.isfinite(self.origin32).all() and np.isfinite(self.inv_h32) and self.inv_h32 > 0):
            raise ValueError("origin and 1/spacing must be finite in float32")
        self._dev = {}

    def on(self, device):
        """{"phi": flat float32 field, "origin", "inv_h", "top": float32 constants of the torch statement} on `device`, made once."""
        import torch
        device = torch.device(device)
        key = str(device if device.index is not None or device.type != "cuda" else torch.device("cuda", torch.cuda.current_device()))
        hit = self._dev.get(key)
        if hit is None:
            nx, ny, nz = self.shape
            hit = self._dev[key] = dict(
                phi=torch.from_numpy(self.phi.reshape(-1)).to(device),
                origin=torch.from_numpy(self.origin32.copy()).to(device),
                inv_h=torch.tensor(float(self.inv_h32), dtype=torch.float32, device=device),
                top=torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=device))
        return hit


# ---- the field ---------------------------------------------------------------------------------------------------------
def usable_faces(verts, faces):
    """(tris f64 [F', 9], dropped, degenerate): v0, v1, v2 of the faces that the field is built from, in face order."""
    verts, faces = check_mesh(verts, faces)
    tri = verts[faces]                                                      # [F, 3, 3]
    finite = np.isfinite(tri).all(axis=(1, 2))
    tri = tri[finite]
    with np.errstate(all="ignore"):
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        area = np.isfinite(nn) & (nn > 0.0)
    return np.ascontiguousarray(tri[area].reshape(-1, 9)), int((~finite).sum()), int((~area).sum())


def grid_box(verts, grid, pad):
    """(origin f64 [3], h, (nx, ny, nz)) of the contract's box over the finite vertices."""
    grid, pad = int(grid), float(pad)
    if not MIN_GRID <= grid <= MAX_GRID:
        raise ValueError(f"grid = {grid} ({MIN_GRID} to {MAX_GRID})")
    if not (math.isfinite(pad) and pad >= 0.0):
        raise ValueError(f"pad = {pad} (finite and >= 0)")
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    finite = verts[np.isfinite(verts).all(axis=1)]
    if finite.shape[0] == 0:
        raise ValueError("the mesh has no finite vertex")
    lo, hi = finite.min(axis=0), finite.max(axis=0)
    with np.errstate(all="ignore"):
        m = pad * (hi - lo).max()
        origin, top = lo - m, hi + m
        side = top - origin
        h = float(side.max() / (grid - 1))
        if not (math.isfinite(h) and h > 0.0 and np.isfinite(origin).all()):
            raise ValueError(f"the mesh's box {lo.tolist()} .. {hi.tolist()} gives a spacing of {h}: a mesh with some extent expected")
        n = np.ceil(side / h) + 1.0
    return origin, h, tuple(int(v) for v in n)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _pair_terms(p, tris):
    """(dist2, omega) f64 [N, F] of nodes p = (x, y, z) [N, 1] each and faces tris [F, 9]."""
    v0, v1, v2 = ([tris[None, :, 3 * k + j] for j in range(3)] for k in range(3))
    a = [v0[j] - p[j] for j in range(3)]
    b = [v1[j] - p[j] for j in range(3)]
    c = [v2[j] - p[j] for j in range(3)]
    ap, bp, cp = [-x for x in a], [-x for x in b], [-x for x in c]
    e1 = [v1[j] - v0[j] for j in range(3)]
    e2 = [v2[j] - v0[j] for j in range(3)]
    e3 = [v2[j] - v1[j] for j in range(3)]
    d1, d2, d3, d4, d5, d6 = _dot(e1, ap), _dot(e2, ap), _dot(e1, bp), _dot(e2, bp), _dot(e1, cp), _dot(e2, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    s = 1.0 / ((va + vb) + vc)
    v, w = vb * s, vc * s
    q = [ap[j] - (e1[j] * v + e2[j] * w) for j in range(3)]                                   # interior, then the regions last to first
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    sel = (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)
    q = [np.where(sel, bp[j] - w * e3[j], q[j]) for j in range(3)]
    w = d2 / (d2 - d6)
    sel = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0)
    q = [np.where(sel, ap[j] - w * e2[j], q[j]) for j in range(3)]
    sel = (d6 >= 0.0) & (d5 <= d6)
    q = [np.where(sel, cp[j], q[j]) for j in range(3)]
    v = d1 / (d1 - d3)
    sel = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0)
    q = [np.where(sel, ap[j] - v * e1[j], q[j]) for j in range(3)]
    sel = (d3 >= 0.0) & (d4 <= d3)
    q = [np.where(sel, bp[j], q[j]) for j in range(3)]
    sel = (d1 <= 0.0) & (d2 <= 0.0)
    q = [np.where(sel, ap[j], q[j]) for j in range(3)]
    dist2 = _dot(q, q)
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0])
    den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
    return dist2, 2.0 * np.arctan2(det, den)


def field_numpy(tris, origin, h, shape):
    """(phi float32 [nz, ny, nx], winding f64 [nz, ny, nx]) of the usable faces `tris` [F, 9] on the grid."""
    nx, ny, nz = shape
    N, F = nx * ny * nz, tris.shape[0]
    node = np.arange(N, dtype=np.int64)
    pos = [origin[0] + (node % nx).astype(np.float64) * h, origin[1] + ((node // nx) % ny).astype(np.float64) * h,
           origin[2] + (node // (nx * ny)).astype(np.float64) * h]
    best, S = np.full(N, np.inf), np.zeros(N)
    rows = max(1, _PAIRS // max(1, min(F, 256)))
    with np.errstate(all="ignore"):
        for r0 in range(0, N, rows):
            p = [x[r0:r0 + rows, None] for x in pos]
            for f0 in range(0, F, 256):
                dist2, omega = _pair_terms(p, tris[f0:f0 + 256])
                dist2 = np.where(dist2 < np.inf, dist2, np.inf)                # (a NaN never passes the comparison)
                best[r0:r0 + rows] = np.minimum(best[r0:r0 + rows], dist2.min(axis=1))
                for j in range(omega.shape[1]):                                # face order
                    S[r0:r0 + rows] += omega[:, j]
        w = S / FOUR_PI
        mag = np.sqrt(best).astype(np.float32)
    phi = np.where((w > 0.5) & (mag != 0), -mag, mag)
    return phi.reshape(nz, ny, nx), w.reshape(nz, ny, nx)


def field_device(tris, origin, h, shape, device="cuda", winding=False):
    """hgs_mesh_sdf on a float64 device tensor [F, 9]: (phi, winding or None), device tensors [nz, ny, nx]."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(tris, "tris", torch.float64)
    if tris.dim() != 2 or tris.shape[1] != 9:
        raise rt.HgsError(f"tris {tuple(tris.shape)}: [F, 9] expected")
    nx, ny, nz = (int(n) for n in shape)
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > 1024:
        raise rt.HgsError(f"a grid of {nx} x {ny} x {nz} nodes (1 to 1024 an axis)")
    phi = torch.empty((nz, ny, nx), dtype=torch.float32, device=tris.device)
    wn = torch.empty((nz, ny, nx), dtype=torch.float64, device=tris.device) if winding else None
    with torch.cuda.device(tris.device):
        rt.check(rt.lib().hgs_mesh_sdf(rt.current_stream(), tris.shape[0], rt.ptr(tris), float(origin[0]), float(origin[1]),
                                       float(origin[2]), float(h), nx, ny, nz, rt.ptr(phi), rt.ptr(wn)))
    return phi, wn


def build_sdf(verts, faces, grid=128, pad=0.1, device=None, stats=None):
    """The HeadSDF of a mesh.  `stats`, a dict, receives "dropped", "degenerate", "faces" (the usable ones) and, on request by the
    key "winding" being present, the winding numbers f64 [nz, ny, nx]."""
    verts, faces = check_mesh(verts, faces)
    tris, dropped, degenerate = usable_faces(verts, faces)
    if tris.shape[0] == 0:
        raise ValueError(f"no usable face: {faces.shape[0]} face(s), {dropped} with a vertex that is not finite, {degenerate} of zero area")
    origin, h, shape = grid_box(verts, grid, pad)
    want_w = stats is not None and "winding" in stats
    if is_cuda(device):
        import torch
        phi, wn = field_device(torch.from_numpy(tris).to(device), origin, h, shape, device, winding=want_w)
        phi, wn = phi.cpu().numpy(), None if wn is None else wn.cpu().numpy()
    else:
        phi, wn = field_numpy(tris, origin, h, shape)
    if stats is not None:
        stats.update(dropped=dropped, degenerate=degenerate, faces=int(tris.shape[0]))
        if want_w:
            stats["winding"] = wn
    return HeadSDF(origin, h, shape, phi, mesh_faces=faces.shape[0], mesh_verts=verts.shape[0])


# ---- the file ----------------------------------------------------------------------------------------------------------
def save_sdf(path, sdf):
    """Writes head_sdf.npz (np.savez appends .npz to any other ending)."""
    np.savez(path, origin=sdf.origin, spacing=np.float64(sdf.spacing), shape=np.asarray(sdf.shape, np.int64), phi=sdf.phi,
             mesh_faces=np.int64(sdf.mesh_faces), mesh_verts=np.int64(sdf.mesh_verts))


def load_sdf(path):
    """The HeadSDF of a head_sdf.npz; ValueError, in this module's words, for anything else."""
    try:
        with np.load(path, allow_pickle=False) as z:
            if set(z.files) != set(KEYS):
                raise ValueError(f"{path}: keys {sorted(z.files)}, a distance field holds {sorted(KEYS)}")
            data = {k: z[k] for k in KEYS}
    except (OSError, EOFError, KeyError) as e:
        raise ValueError(f"{path}: not a head distance field ({e})") from None
    except ValueError as e:
        if str(e).startswith(str(path)):
            raise
        raise ValueError(f"{path}: not a head distance field ({e})") from None
    o, s, sh, phi = data["origin"], data["spacing"], data["shape"], data["phi"]
    if o.shape != (3,) or o.dtype != np.float64 or s.shape != () or s.dtype != np.float64 or sh.shape != (3,) or sh.dtype.kind not in "iu" \
            or phi.dtype != np.float32 or phi.ndim != 3 or any(data[k].shape != () or data[k].dtype.kind not in "iu" for k in KEYS[4:]):
        raise ValueError(f"{path}: origin f64 [3], spacing f64, shape int [3], phi float32 [nz, ny, nx] and two integer counts expected")
    try:
        return HeadSDF(o, float(s), tuple(int(v) for v in sh), phi, int(data["mesh_faces"]), int(data["mesh_verts"]))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def scene_sdf_path(source_path):
    return os.path.join(source_path, FILE)


# ---- the term: numpy path ----------------------------------------------------------------------------------------------
def _points32(points):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points of shape {points.shape}: [E, 3] expected")
    return np.ascontiguousarray(points, dtype=np.float32)


def _lerp(u, v, f):
    return u + f * (v - u)


def trilinear(points, sdf):
    """(in_range bool [E], d, gx, gy, gz f32 [E]) of the contract's term up to the interpolated distance and its gradient; rows out
    of range hold the values of some valid cell (scene/strand_collide.py samples the field by this statement too)."""
    p = _points32(points)
    nx, ny, nz = sdf.shape
    k = sdf.inv_h32
    with np.errstate(all="ignore"):
        t = (p - sdf.origin32[None, :]) * k
        top = np.array([nx - 1, ny - 1, nz - 1], np.float32)
        ok = (np.isfinite(t) & (t >= 0) & (t < top[None, :])).all(axis=1)
        t = np.where(ok[:, None], t, np.float32(0))
        fl = np.floor(t)
        i = fl.astype(np.int64)
        f = t - fl
        i1 = np.minimum(i + 1, np.array([nx - 1, ny - 1, nz - 1]))              # (rows out of range: any valid address)
        phi = sdf.phi
        c = {(x, y, z): phi[(i1 if z else i)[:, 2], (i1 if y else i)[:, 1], (i1 if x else i)[:, 0]] for x in (0, 1) for y in (0, 1) for z in (0, 1)}
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        c00, c10 = _lerp(c[0, 0, 0], c[1, 0, 0], fx), _lerp(c[0, 1, 0], c[1, 1, 0], fx)
        c01, c11 = _lerp(c[0, 0, 1], c[1, 0, 1], fx), _lerp(c[0, 1, 1], c[1, 1, 1], fx)
        d = _lerp(_lerp(c00, c10, fy), _lerp(c01, c11, fy), fz)
        gx = _lerp(_lerp(c[1, 0, 0] - c[0, 0, 0], c[1, 1, 0] - c[0, 1, 0], fy), _lerp(c[1, 0, 1] - c[0, 0, 1], c[1, 1, 1] - c[0, 1, 1], fy), fz) * k
        gy = _lerp(_lerp(c[0, 1, 0] - c[0, 0, 0], c[1, 1, 0] - c[1, 0, 0], fx), _lerp(c[0, 1, 1] - c[0, 0, 1], c[1, 1, 1] - c[1, 0, 1], fx), fz) * k
        gz = _lerp(_lerp(c[0, 0, 1] - c[0, 0, 0], c[1, 0, 1] - c[1, 0, 0], fx), _lerp(c[0, 1, 1] - c[0, 1, 0], c[1, 1, 1] - c[1, 1, 0], fx), fy) * k
    assert d.dtype == np.float32 and gx.dtype == np.float32 and gy.dtype == np.float32 and gz.dtype == np.float32
    return ok, d, gx, gy, gz


def sample(points, sdf, margin=0.0):
    """(pen f32 [E], g f32 [E, 3], d f32 [E], in_range bool [E]) of the contract's term; d = +inf out of range."""
    ok, d, gx, gy, gz = trilinear(points, sdf)
    margin = np.float32(margin)
    with np.errstate(all="ignore"):
        r = margin - d
        on = ok & (r > 0)
        pen = np.where(on, r * r, np.float32(0))
        s = np.float32(-2.0) * r
        g = np.where(on[:, None], np.stack([s * gx, s * gy, s * gz], axis=1), np.float32(0))
        d = np.where(ok, d, np.float32(np.inf))
    assert pen.dtype == np.float32 and g.dtype == np.float32 and d.dtype == np.float32
    return pen, g, d, ok


def penalty(points, sdf, margin=0.0, upstream=1.0):
    """(L float32, dL/dpoints f32 [E, 3]) of the contract's term for an upstream gradient."""
    pen, g, _, _ = sample(points, sdf, margin)
    E = pen.shape[0]
    if E == 0:
        return np.float32(0), g
    L = np.float32(pen.astype(np.float64).sum() / np.float64(E))
    return L, g * (np.float32(upstream) / np.float32(E))


def penetration_stats(points, sdf, device=None):
    """{"joints", "inside", "share", "deepest", "mean_depth"} of the joints `points` [E, 3] against the field: a joint is inside where it
    is in range and the interpolated distance is negative; depths are -d, in scene units.  The same sampling statement on both paths
    (device: hgs_head_penalty_forward with margin 0)."""
    if is_cuda(device):
        import torch
        from hgs_runtime.fused import head_penalty
        pts = torch.as_tensor(_points32(points)).to(device)
        info = {}
        head_penalty(pts, sdf, 0.0, info)
        d = info["dist"].cpu().numpy()
    else:
        d = sample(points, sdf, 0.0)[2]
    E = int(d.shape[0])
    depth = -d[d < 0].astype(np.float64)
    n = int(depth.shape[0])
    return dict(joints=E, inside=n, share=(n / E if E else 0.0), deepest=(float(depth.max()) if n else 0.0),
                mean_depth=(float(depth.mean()) if n else 0.0))
