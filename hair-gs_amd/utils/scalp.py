"""The scalp of a capture, labelled on its head mesh from the hair masks: a point of the mesh's surface is scalp where enough of the
views that actually see it -- facing it, and not hidden behind another part of the mesh -- find it under hair.  The kept points are the
capture's strand roots (init_scalp.py is the scene driver and writes head_reconstruction_data.npz; the reference takes FLAME's fixed
scalp region, which ignores where this person's hairline is, and has nothing for another head model).

The contract (this module's numpy path, csrc/hgs_scalp.hip and the loop restatement in tests/scalp_reference.py state the same thing).
All arithmetic is float64 with one rounding per operation, in exactly the order written (the kernel file is built with
-ffp-contract=off).  Views are utils.views.View records; the camera coordinates xc, yc, zc and u, v, seen, px, py of a point are
those of utils/views.py's projection contract.

Mesh.  verts f64 [NV, 3] (any values, NaN included), faces an integer array [F, 3] with 0 <= index < NV; anything else raises
ValueError.

Depth map of view k, Z_k f64 [H, W], +inf to begin with.  For every face (i0, i1, i2), with (xc_i, yc_i, zc_i) and (u_i, v_i) of its
three vertices:
    the face is dropped, and counted, when a zc_i is not > 0 or a u_i or v_i is not finite (no near-plane clipping: a stated limit)
    pixel (px, py) is sampled at its centre (cx, cy) = (px + 0.5, py + 0.5)
    candidates:  max(0, ceil(min u - 0.5)) <= px <= min(W - 1, floor(max u - 0.5)),  likewise py from v and H
    E0 = (u2 - u1)*(cy - v1) - (v2 - v1)*(cx - u1)          (edge v1 -> v2)
    E1 = (u0 - u2)*(cy - v2) - (v0 - v2)*(cx - u2)          (edge v2 -> v0)
    E2 = (u1 - u0)*(cy - v0) - (v1 - v0)*(cx - u0)          (edge v0 -> v1)
    S  = (E0 + E1) + E2
    covered  iff  S != 0  and  (every E >= 0  or  every E <= 0)       (both windings, no culling, edges inclusive; a NaN: not covered)
    iz = (E0*(1/zc0) + E1*(1/zc1)) + E2*(1/zc2),   z = S/iz
    Z_k[py, px] = min(Z_k[py, px], z)   where covered and z is finite and > 0
Two faces that share an edge both cover a centre on it, and a minimum does not mind.  A minimum is also independent of the order of
the faces and of how the work is split: the numpy path and the kernel give equal bits.

Samples.  surface_samples(verts, faces, spacing) returns (points, normals), f64 [n, 3].  The points begin with the NV vertices; a
vertex's normal is the sum of the cross products (v1 - v0) x (v2 - v0) of its faces, added in face order, not normalised.  With
spacing > 0 every face then adds, in face order, the centroids of the m*m sub-triangles of its regular m-subdivision,
m = min(64, ceil(L/spacing)) with L its longest edge (m = 0, nothing, for L = 0 or not finite): first the sub-triangles that stand
like the face, p = (v0 + ((3i + 1)/(3m))*(v1 - v0)) + ((3j + 1)/(3m))*(v2 - v0) for i = 0..m-1, j = 0..m-1-i, then the upside-down
ones, with (3i + 2) and (3j + 2), for i = 0..m-2, j = 0..m-2-i.  Their normal is the face's cross product.  Host numpy plumbing
around the kernels, the same on both devices.

Vote of the sample (p, n) in view k, with seen, px, py, xc, yc, zc of p as above:
    nc_r = (R_r0*n0 + R_r1*n1) + R_r2*n2                   (the normal in camera coordinates)
    d  = -((nc0*xc + nc1*yc) + nc2*zc)
    nn = (nc0*nc0 + nc1*nc1) + nc2*nc2,   pp = (xc*xc + yc*yc) + zc*zc
    facing   iff  d > 0  and  d*d >= (min_cos*min_cos)*(nn*pp)        (the cosine between normal and view ray, without a root)
    visible  iff  seen and facing and zc <= Z_k[py, px] + depth_tol   (a pixel no face covers holds +inf: visible)
    vis += visible,   hits += visible and mask[py, px] != 0
0 <= min_cos <= 1; depth_tol is finite and >= 0.  vis and hits are int32 sums: exact, and independent of the order of the views.

Keep rule: utils.carve.keep(vis, hits, min_views, min_percent), with `vis` in the place of the carving's `seen`.

label_scalp(verts, faces, views, masks, spacing, min_cos, depth_tol, min_views, min_percent) returns (scalp_points, vis, hits, kept):
the samples, their votes against the mesh's own depth maps, and the kept samples' points.  A depth map costs 8 bytes a pixel, so the
device path walks the views in batches under a byte budget (view_batches) and adds the integer counts: the result does not depend on
the batching.

Known limits.  Hair that hangs in front of skin (a fringe, long hair over the cheek) votes that skin as scalp in the views where it
does: min_percent is the knob for it, not a cure.  depth_tol is absolute, in scene units; it exists because a sample ON the surface
is compared with the depth interpolated at a pixel centre next to it, and at a grazing angle the two differ by more than rounding.
A face that crosses a camera's plane is dropped in that view, so what it would hide there counts as visible.

device=None: numpy.  device="cuda": the kernels.  The caller chooses; neither falls back to the other (utils/carve.py's convention)."""
import math

import numpy as np

from utils import carve
from utils.views import camera, check_count, check_views, image_point, is_cuda, pack, pixel, upload_planes

MAX_VERTS = 1 << 24
MAX_FACES = 1 << 24
MAX_SUBDIVISION = 64
DEPTH_BUDGET = 1 << 30          # bytes of depth maps that the device path holds at a time
_CHUNK = 1 << 20                # candidate pixels per numpy pass


def check_mesh(verts, faces):
    """(verts f64 [NV, 3], faces int64 [F, 3]) or ValueError."""
    try:
        verts = np.asarray(verts, np.float64)
    except (TypeError, ValueError):
        raise ValueError("verts must be a float array [NV, 3]") from None
    faces = np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts of shape {verts.shape}: [NV, 3] expected")
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError(f"faces of shape {faces.shape} and type {faces.dtype}: an integer array [F, 3] expected")
    if verts.shape[0] > MAX_VERTS or faces.shape[0] > MAX_FACES:
        raise ValueError(f"{verts.shape[0]} vertices and {faces.shape[0]} faces (at most {MAX_VERTS} and {MAX_FACES})")
    faces = faces.astype(np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= verts.shape[0]):
        raise ValueError(f"a face index is out of range of the {verts.shape[0]} vertices")
    return np.ascontiguousarray(verts), np.ascontiguousarray(faces)


def _check_knobs(min_cos, depth_tol):
    min_cos, depth_tol = float(min_cos), float(depth_tol)
    if not 0.0 <= min_cos <= 1.0:
        raise ValueError(f"min_cos = {min_cos} (0 to 1)")
    if not (math.isfinite(depth_tol) and depth_tol >= 0.0):
        raise ValueError(f"depth_tol = {depth_tol} (finite and >= 0)")
    return min_cos, depth_tol


def _check_sizes(views):
    check_count(len(views))
    for k, v in enumerate(views):
        if int(v.W) < 1 or int(v.H) < 1:
            raise ValueError(f"view {k} ({v.name}): {v.W} x {v.H} pixels")


def _check_depth(views, depth):
    if len(depth) != len(views):
        raise ValueError("one depth map per view")
    for k, v in enumerate(views):
        if depth[k].dtype != np.float64 or depth[k].shape != (v.H, v.W):
            raise ValueError(f"view {k} ({v.name}): a float64 depth map of {v.W} x {v.H} pixels expected, got {depth[k].dtype} {depth[k].shape}")


# ---- numpy path ------------------------------------------------------------------------------------------------------
def _depth_view(view, verts, faces):
    """(Z f64 [H, W], dropped) of one view.  Every candidate (face, pixel) pair is a row of flat arrays, _CHUNK of them at a time."""
    W, H = int(view.W), int(view.H)
    Z = np.full(H * W, np.inf)
    with np.errstate(all="ignore"):
        xc, yc, zc = camera(view, verts[:, 0], verts[:, 1], verts[:, 2])
        u, v = image_point(view, xc, yc, zc)
        ok = ((zc > 0.0) & np.isfinite(u) & np.isfinite(v))[faces].all(axis=1)
        f = faces[ok]
        U, Vv, IZ = u[f], v[f], 1.0 / zc[f]
        x0 = np.maximum(0.0, np.ceil(U.min(axis=1) - 0.5))
        x1 = np.minimum(W - 1.0, np.floor(U.max(axis=1) - 0.5))
        y0 = np.maximum(0.0, np.ceil(Vv.min(axis=1) - 0.5))
        y1 = np.minimum(H - 1.0, np.floor(Vv.max(axis=1) - 0.5))
        has = (x0 <= x1) & (y0 <= y1)
        U, Vv, IZ = U[has], Vv[has], IZ[has]
        x0, y0 = x0[has].astype(np.int64), y0[has].astype(np.int64)
        bw, bh = x1[has].astype(np.int64) - x0 + 1, y1[has].astype(np.int64) - y0 + 1
        a = [U[:, 2] - U[:, 1], U[:, 0] - U[:, 2], U[:, 1] - U[:, 0]]             # edges v1 -> v2, v2 -> v0, v0 -> v1
        b = [Vv[:, 2] - Vv[:, 1], Vv[:, 0] - Vv[:, 2], Vv[:, 1] - Vv[:, 0]]
        start = (1, 2, 0)                                                          # the vertex each edge starts at
        ends = np.cumsum(bw * bh)
        first = 0
        while first < ends.size:
            base = int(ends[first - 1]) if first else 0
            last = max(first + 1, int(np.searchsorted(ends, base + _CHUNK, side="right")))
            n = (bw * bh)[first:last]
            fi = np.repeat(np.arange(first, last), n)
            local = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(ends[first:last] - n - base, n)
            px, py = x0[fi] + local % bw[fi], y0[fi] + local // bw[fi]
            cx, cy = px + 0.5, py + 0.5
            E = [a[k][fi] * (cy - Vv[fi, start[k]]) - b[k][fi] * (cx - U[fi, start[k]]) for k in range(3)]
            S = (E[0] + E[1]) + E[2]
            covered = (S != 0.0) & (((E[0] >= 0.0) & (E[1] >= 0.0) & (E[2] >= 0.0)) | ((E[0] <= 0.0) & (E[1] <= 0.0) & (E[2] <= 0.0)))
            z = S / ((E[0] * IZ[fi, 0] + E[1] * IZ[fi, 1]) + E[2] * IZ[fi, 2])
            put = covered & np.isfinite(z) & (z > 0.0)
            np.minimum.at(Z, (py * W + px)[put], z[put])
            first = last
    return Z.reshape(H, W), int(faces.shape[0] - ok.sum())


def depth_numpy(verts, faces, views):
    verts, faces = check_mesh(verts, faces)
    _check_sizes(views)
    maps, dropped = [], 0
    for view in views:
        Z, d = _depth_view(view, verts, faces)
        maps.append(Z)
        dropped += d
    return maps, dropped


def _samples(points, normals):
    points, normals = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError(f"points {points.shape} and normals {normals.shape}: two arrays [N, 3] expected")
    return np.ascontiguousarray(points), np.ascontiguousarray(normals)


def votes_numpy(points, normals, views, masks, depth, min_cos, depth_tol):
    points, normals = _samples(points, normals)
    check_views(views, masks)
    _check_depth(views, depth)
    min_cos, depth_tol = _check_knobs(min_cos, depth_tol)
    N = points.shape[0]
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    n0, n1, n2 = normals[:, 0], normals[:, 1], normals[:, 2]
    vis, hits = np.zeros(N, np.int32), np.zeros(N, np.int32)
    c2 = min_cos * min_cos
    for k, view in enumerate(views):
        R = view.R
        xc, yc, zc = camera(view, x, y, z)
        seen, py, px = pixel(view, xc, yc, zc)
        with np.errstate(all="ignore"):
            nc = [(R[r, 0] * n0 + R[r, 1] * n1) + R[r, 2] * n2 for r in range(3)]
            d = -((nc[0] * xc + nc[1] * yc) + nc[2] * zc)
            nn = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]
            pp = (xc * xc + yc * yc) + zc * zc
            facing = (d > 0.0) & (d * d >= c2 * (nn * pp))
            visible = seen & facing & (zc <= depth[k][py, px] + depth_tol)
        vis += visible
        hits += visible & (masks[k][py, px] != 0)
    return vis, hits


def surface_samples(verts, faces, spacing):
    """(points, normals) f64 [n, 3]: the vertices, then (spacing > 0) the sub-triangle centroids of every face."""
    verts, faces = check_mesh(verts, faces)
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing >= 0.0):
        raise ValueError(f"spacing = {spacing} (finite and >= 0)")
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        fn = np.cross(e1, e2).reshape(-1, 3)
        vn = np.zeros_like(verts)
        np.add.at(vn, faces.reshape(-1), np.repeat(fn, 3, axis=0))              # (flat order: face by face)
        if spacing == 0.0 or faces.shape[0] == 0:
            return verts.copy(), vn
        L = np.sqrt(np.maximum(np.maximum((e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1)), ((v2 - v1) ** 2).sum(axis=1)))
        m = np.where(np.isfinite(L), np.minimum(float(MAX_SUBDIVISION), np.ceil(L / spacing)), 0.0).astype(np.int64)
    offset = np.concatenate([[0], np.cumsum(m * m)])                             # a face's first row: face order
    out_p, out_n = np.empty((int(offset[-1]), 3)), np.empty((int(offset[-1]), 3))
    for mm in (int(q) for q in np.unique(m[m > 0])):                             # one barycentric table per subdivision
        ab = [((3 * i + 1) / (3 * mm), (3 * j + 1) / (3 * mm)) for i in range(mm) for j in range(mm - i)]
        ab += [((3 * i + 2) / (3 * mm), (3 * j + 2) / (3 * mm)) for i in range(mm - 1) for j in range(mm - 1 - i)]
        ab = np.array(ab, np.float64)
        idx = np.flatnonzero(m == mm)
        with np.errstate(all="ignore"):
            p = (v0[idx, None, :] + ab[None, :, 0, None] * e1[idx, None, :]) + ab[None, :, 1, None] * e2[idx, None, :]
        rows = (offset[idx][:, None] + np.arange(mm * mm)[None, :]).reshape(-1)
        out_p[rows] = p.reshape(-1, 3)
        out_n[rows] = np.broadcast_to(fn[idx, None, :], p.shape).reshape(-1, 3)
    return np.concatenate([verts, out_p]), np.concatenate([vn, out_n])


# ---- device path -----------------------------------------------------------------------------------------------------
def view_batches(views, budget=None):
    """[(first, last), ...]: runs of consecutive views whose depth maps (8 bytes a pixel) fit `budget` bytes together; a view larger
    than the budget is a run of its own."""
    budget = DEPTH_BUDGET if budget is None else int(budget)
    out, first, used = [], 0, 0
    for k, v in enumerate(views):
        need = 8 * int(v.W) * int(v.H)
        if k > first and used + need > budget:
            out.append((first, k))
            first, used = k, 0
        used += need
    if len(views) > first:
        out.append((first, len(views)))
    return out


def depth_device(verts, faces, packed):
    """hgs_scalp_depth on device tensors (verts float64 [NV, 3], faces int32 [F, 3]) and the packed views: (depth, dropped) -- one
    float64 tensor that holds view k's map at element offset records[k].mask_offset, and the number of dropped (face, view) pairs."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(verts, "verts", torch.float64)
    rt.require_device_buffer(faces, "faces", torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise rt.HgsError(f"verts {tuple(verts.shape)} and faces {tuple(faces.shape)}: [NV, 3] and [F, 3] expected")
    total = max(r.mask_offset + r.W * r.H for r in packed.records)
    depth = torch.empty(total, dtype=torch.float64, device=verts.device)
    V = rt.scalp_check(packed.records, packed.views_dev, packed.masks_dev, depth, faces=faces, n_verts=verts.shape[0])
    dropped = torch.empty(1, dtype=torch.int64, device=verts.device)
    with torch.cuda.device(verts.device):
        rt.check(rt.lib().hgs_scalp_depth(rt.current_stream(), verts.shape[0], rt.ptr(verts), faces.shape[0], rt.ptr(faces), V,
                                          rt.ptr(packed.views_dev), rt.ptr(depth), rt.ptr(dropped)))
    return depth, int(dropped.item())


def votes_device(points, normals, packed, depth, min_cos, depth_tol):
    """hgs_scalp_votes on float64 device tensors [N, 3]: (vis, hits), int32 tensors on their device."""
    import torch
    import hgs_runtime as rt
    rt.require_device_buffer(points, "points", torch.float64)
    rt.require_device_buffer(normals, "normals", torch.float64)
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise rt.HgsError(f"points {tuple(points.shape)} and normals {tuple(normals.shape)}: two tensors [N, 3] expected")
    V = rt.scalp_check(packed.records, packed.views_dev, packed.masks_dev, depth)
    N = points.shape[0]
    vis = torch.empty(N, dtype=torch.int32, device=points.device)
    hits = torch.empty(N, dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        rt.check(rt.lib().hgs_scalp_votes(rt.current_stream(), N, rt.ptr(points), rt.ptr(normals), V, rt.ptr(packed.views_dev),
                                          rt.ptr(packed.masks_dev), rt.ptr(depth), float(min_cos), float(depth_tol), rt.ptr(vis), rt.ptr(hits)))
    return vis, hits


def _upload_mesh(verts, faces, device):
    import torch
    return torch.from_numpy(verts).to(device), torch.from_numpy(faces.astype(np.int32)).to(device)


def _split(depth, records):
    """The host maps [H, W] of a depth tensor."""
    flat = depth.cpu().numpy()
    return [flat[r.mask_offset:r.mask_offset + r.W * r.H].reshape(r.H, r.W).copy() for r in records]


# ---- host-array entry points -----------------------------------------------------------------------------------------
def depth_maps(verts, faces, views, device=None, budget=None):
    """(maps, dropped): the depth map f64 [H, W] of every view, host arrays, and the number of dropped (face, view) pairs."""
    if not is_cuda(device):
        return depth_numpy(verts, faces, views)
    verts, faces = check_mesh(verts, faces)
    _check_sizes(views)
    v_dev, f_dev = _upload_mesh(verts, faces, device)
    maps, dropped = [], 0
    for a, b in view_batches(views, budget):
        packed = pack(views[a:b], [np.zeros((v.H, v.W), np.uint8) for v in views[a:b]], None, device)
        depth, d = depth_device(v_dev, f_dev, packed)
        maps += _split(depth, packed.records)
        dropped += d
    return maps, dropped


def scalp_votes(points, normals, views, masks, depth, min_cos, depth_tol, device=None, budget=None):
    """(vis, hits) int32 [N], host arrays; `depth`: the views' maps, host arrays as depth_maps returns them."""
    if not is_cuda(device):
        return votes_numpy(points, normals, views, masks, depth, min_cos, depth_tol)
    import torch
    points, normals = _samples(points, normals)
    check_views(views, masks)
    _check_depth(views, depth)
    p_dev, n_dev = torch.from_numpy(points).to(device), torch.from_numpy(normals).to(device)
    vis = torch.zeros(points.shape[0], dtype=torch.int32, device=device)
    hits = torch.zeros_like(vis)
    for a, b in view_batches(views, budget):
        packed = pack(views[a:b], masks[a:b], None, device)
        d_dev = upload_planes(depth[a:b], device)
        v, h = votes_device(p_dev, n_dev, packed, d_dev, min_cos, depth_tol)
        vis += v
        hits += h
    return vis.cpu().numpy(), hits.cpu().numpy()


def label_scalp(verts, faces, views, masks, spacing, min_cos, depth_tol, min_views, min_percent, device=None, budget=None, stats=None):
    """(scalp_points f64 [n, 3], vis, hits int32 [N], kept bool [N]) over the N samples of surface_samples(verts, faces, spacing).
    `stats`, a dict, receives "dropped": the (face, view) pairs that the depth maps left out."""
    verts, faces = check_mesh(verts, faces)
    check_views(views, masks)
    min_views, min_percent = carve.check_rule(min_views, min_percent)
    points, normals = surface_samples(verts, faces, spacing)
    if not is_cuda(device):
        depth, dropped = depth_numpy(verts, faces, views)
        vis, hits = votes_numpy(points, normals, views, masks, depth, min_cos, depth_tol)
    else:
        import torch
        v_dev, f_dev = _upload_mesh(verts, faces, device)
        p_dev, n_dev = torch.from_numpy(points).to(device), torch.from_numpy(normals).to(device)
        vis_dev = torch.zeros(points.shape[0], dtype=torch.int32, device=device)
        hits_dev = torch.zeros_like(vis_dev)
        dropped = 0
        for a, b in view_batches(views, budget):
            packed = pack(views[a:b], masks[a:b], None, device)
            depth, d = depth_device(v_dev, f_dev, packed)
            v, h = votes_device(p_dev, n_dev, packed, depth, min_cos, depth_tol)
            vis_dev += v
            hits_dev += h
            dropped += d
        vis, hits = vis_dev.cpu().numpy(), hits_dev.cpu().numpy()
    kept = carve.keep(vis, hits, min_views, min_percent)
    if stats is not None:
        stats["dropped"] = dropped
    return points[kept], vis, hits, kept
