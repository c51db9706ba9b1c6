"""Line / triangle rasterizer of the dataset synthesis (the reference renders its captures with OpenGL in
scene/OpenGLRenderer.py; OpenGL is not available where this project runs).  scene/OpenGLRenderer.py keeps the reference's class
names over this module.

The contract (DESIGN.md "Dataset synthesis").  Both backends, device=None (numpy) and device="cuda" (csrc/hgs_raster.hip), give
bit-identical images, because every decision is made in integers and all arithmetic runs in float64, operation by operation, in the
order written here.  Inputs are cast to float32 first, as the reference's VBOs and uniforms are.
  Vertices (per view): p_w = M [p, 1]; c = P (Vw p_w), each row summed left to right; Vw is the OpenGL view matrix
    diag(1, -1, -1, 1) w2c and P colmap_camera_to_projection_matrix.  ndc = c.xyz / c.w; x_w = (ndc.x 0.5 + 0.5) W,
    y_w = (ndc.y 0.5 + 0.5) H, z_w = ndc.z 0.5 + 0.5; X = rint(256 x_w), Y = rint(256 y_w) (half to even, int64).
    A primitive is DROPPED and counted when one of its vertices has c.w <= 0, |c.z| > c.w, or |x_w| or |y_w| > 2^14 (GL would
    clip it).  Window rows count from the bottom: image row = H - 1 - j.  Pixel (i, j) has its centre at (256 i + 128, 256 j + 128).
  Triangles: A = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0); A <= 0 is culled (GL_BACK, counter-clockwise front faces; degenerate ones too).
    E_k is the edge function of the edge opposite vertex k (E0: v1 -> v2, E1: v2 -> v0, E2: v0 -> v1, E(a -> b) =
    (Xb-Xa)(Py-Ya) - (Yb-Ya)(Px-Xa)).  Covered: every E_k > 0, or == 0 on a left edge (dY < 0) or a top edge (dY == 0, dX < 0).
    b_k = E_k / A; z = (b0 z0 + b1 z1) + b2 z2; q_k = b_k (1 / w_k); attr = ((q0 a0 + q1 a1) + q2 a2) / ((q0 + q1) + q2).
  Lines: width w = max(1, rint(line_width)).  x-major (|dX| >= |dY|): one fragment column per pixel column whose centre Cx lies on
    the half-open interval from Xa (included) to Xb (excluded); Yc = Ya + floor((Cx-Xa)(Yb-Ya) / (Xb-Xa)) (integer floor division,
    divisor made positive); j0 = floor(Yc / 256); rows j0 - (w-1)//2 ... j0 - (w-1)//2 + w - 1.  y-major: x and y swapped.
    t = (Cx-Xa) / (Xb-Xa); z = (1-t) za + t zb; q_a = (1-t) / w_a, q_b = t / w_b; attr = (q_a a_a + q_b a_b) / (q_a + q_b).
    Zero-length lines give nothing.  Pixels outside the viewport are discarded (lines and triangles).
  Depth: d = rint(z (2^24 - 1)), discarded when d >= 2^24 - 1 (GL_LESS against the cleared 1.0).  key = (d << 32) | draw_index,
    draw_index counting the primitives of the SELECTED models in list order, then in primitive order; the smallest key wins (GL_LESS
    with draws in submission order), whatever order the fragments arrive in.
  Shading of the winner: the reference's fragment shader, normals through inv(M[:3,:3]).T.  n^ = n / sqrt(n.n) (n.n == 0, or a
    light at the fragment: no diffuse term); l^ = (L - p) / |L - p|; cos = (n^x l^x + n^y l^y) + n^z l^z;
    light = ka amb + (kd max(cos, 0)) dif; out = light color (unlit: out = color); byte = floor(clamp(out, 0, 1) 255 + 0.5).
    Alpha is dropped.  Pixels without a fragment take `background` (bytes by the same rule).
  Gray (return_gray): OpenCV's 8-bit RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14 (utils.vision.to_gray).
Not pinned: pixel parity with OpenGL (GL clips instead of dropping, rasterizes in its own fixed point and shades in float32)."""
import numpy as np

__all__ = ["MeshModel", "Lighting", "render_views", "MAX_MODELS", "TILE"]

MAX_MODELS = 64          # models per render (csrc/hgs_raster.hip HGS_RASTER_MAX_MODELS)
TILE = 32                # screen tile of the device path
_DMAX = (1 << 24) - 1
_LIM = float(1 << 14)
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


class MeshModel:
    """One draw: vertices [N, 3] with edges [E, 2] (GL_LINES) or faces [F, 3] (GL_TRIANGLES), never both.  colors: one per vertex,
    or one row tiled to every vertex (default white); normals: one per vertex (default ones); model: 4x4 row-major."""

    def __init__(self, verts, colors=None, normals=None, edges=None, faces=None, model=np.eye(4), use_lighting=True, line_width=1.0,
                 ka=0.5, kd=0.5):
        if (edges is None) == (faces is None):
            raise ValueError("give exactly one of edges or faces")
        verts = np.asarray(verts)
        if verts.ndim != 2 or verts.shape[1] != 3:
            raise ValueError(f"verts must be [N, 3], got {verts.shape}")
        self.vertices = verts.astype(np.float32)
        idx = np.asarray(edges if edges is not None else faces)
        k = 2 if edges is not None else 3
        if idx.size and (idx.ndim != 2 or idx.shape[1] != k):
            raise ValueError(f"{'edges' if k == 2 else 'faces'} must be [n, {k}], got {idx.shape}")
        idx = idx.reshape(-1, k).astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= verts.shape[0]):
            raise ValueError("an index is out of range of the vertices")
        self.indices = idx.astype(np.uint32)
        self.kind = k
        if colors is None:
            colors = np.array([1, 1, 1, 1])
        colors = np.asarray(colors)
        if colors.ndim == 1 or colors.shape[0] != verts.shape[0]:      # (one row: tiled even when its length is N)
            colors = np.tile(colors, (verts.shape[0], 1))
        self.colors = colors.astype(np.float32)
        if normals is None:
            normals = np.ones(verts.shape)
        self.normals = np.asarray(normals).astype(np.float32)
        self.model = np.asarray(model).astype(np.float32)
        self.use_lighting = bool(use_lighting)
        self.line_width = line_width
        self.ka = ka
        self.kd = kd

    @property
    def width(self):
        return max(1, int(np.rint(self.line_width)))

    def world(self):
        """(p_w [N, 4], n_w [N, 3], rgb [N, 3]) in float64: the view-independent part of the vertex stage, shared by both backends."""
        M = self.model.astype(np.float64)
        p = self.vertices.astype(np.float64)
        pw = np.empty((p.shape[0], 4))
        for r in range(4):
            pw[:, r] = ((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]
        N = np.linalg.inv(M[:3, :3]).T
        n = self.normals.astype(np.float64)
        nw = np.empty((n.shape[0], 3))
        for r in range(3):
            nw[:, r] = (N[r, 0] * n[:, 0] + N[r, 1] * n[:, 1]) + N[r, 2] * n[:, 2]
        return pw, nw, self.colors[:, :3].astype(np.float64)


class Lighting:
    def __init__(self, light_pos=np.array([10, 10, 10]), diffuse_color=np.zeros(4), ambient_color=np.zeros(4)):
        self.light_pos = np.asarray(light_pos).astype(np.float32)
        self.diffuse_color = np.asarray(diffuse_color).astype(np.float32)
        self.ambient_color = np.asarray(ambient_color).astype(np.float32)

    def packed(self):
        """float64 [9]: light position, ambient rgb, diffuse rgb."""
        return np.concatenate([self.light_pos[:3], self.ambient_color[:3], self.diffuse_color[:3]]).astype(np.float64)


def unorm8(v):
    return np.floor(np.clip(np.asarray(v, np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def _floordiv(a, b):
    return np.floor_divide(a, b)


def _ceildiv(a, b):
    return -np.floor_divide(-a, b)


def _mat_rows(Mx, v):
    """Rows of a 4x4 float64 matrix applied to v [N, 4], each summed left to right."""
    out = np.empty_like(v)
    for r in range(4):
        out[:, r] = ((Mx[r, 0] * v[:, 0] + Mx[r, 1] * v[:, 1]) + Mx[r, 2] * v[:, 2]) + Mx[r, 3] * v[:, 3]
    return out


def _vertex_stage(pw, view, proj, W, H):
    e = _mat_rows(view, pw)
    c = _mat_rows(proj, e)
    cw = c[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        xw = ((c[:, 0] / cw) * 0.5 + 0.5) * W
        yw = ((c[:, 1] / cw) * 0.5 + 0.5) * H
        zw = (c[:, 2] / cw) * 0.5 + 0.5
        ok = (cw > 0) & (np.abs(c[:, 2]) <= cw) & (np.abs(xw) <= _LIM) & (np.abs(yw) <= _LIM)
    X = np.where(ok, np.rint(256.0 * np.where(ok, xw, 0.0)), 0).astype(np.int64)
    Y = np.where(ok, np.rint(256.0 * np.where(ok, yw, 0.0)), 0).astype(np.int64)
    return X, Y, zw, cw, ok


def _depth_key(z, draw):
    d = np.rint(z * float(_DMAX)).astype(np.int64)
    d = np.maximum(d, 0)
    keep = d < _DMAX
    return (d.astype(np.uint64) << np.uint64(32)) | draw.astype(np.uint64), keep


def _line_setup(Ua, Va, Ub, Vb):
    """Major-axis pixel range [k0, k1] of a line in (major U, minor V) coordinates."""
    fwd = Ua <= Ub
    k0 = np.where(fwd, _ceildiv(Ua - 128, 256), _floordiv(Ub - 128, 256) + 1)
    k1 = np.where(fwd, _ceildiv(Ub - 128, 256) - 1, _floordiv(Ua - 128, 256))
    return k0, k1


def _line_minor(Ua, Va, Ub, Vb, Cu):
    dU, dV = Ub - Ua, Vb - Va
    num = (Cu - Ua) * dV
    num = np.where(dU < 0, -num, num)
    return Va + _floordiv(num, np.abs(dU))


def _lines(X, Y, z, cw, ok, a, b, draw, width, W, H):
    """Fragments (flat window pixel, key) of lines a -> b."""
    good = ok[a] & ok[b]
    Xa, Ya, Xb, Yb = X[a], Y[a], X[b], Y[b]
    xmaj = np.abs(Xb - Xa) >= np.abs(Yb - Ya)
    Ua, Va = np.where(xmaj, Xa, Ya), np.where(xmaj, Ya, Xa)
    Ub, Vb = np.where(xmaj, Xb, Yb), np.where(xmaj, Yb, Xb)
    Wu, Wv = np.where(xmaj, W, H), np.where(xmaj, H, W)
    k0, k1 = _line_setup(Ua, Va, Ub, Vb)
    k0, k1 = np.maximum(k0, 0), np.minimum(k1, Wu - 1)
    n = np.where(good, np.maximum(k1 - k0 + 1, 0), 0)
    li = np.repeat(np.arange(a.shape[0]), n)
    if li.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    k = k0[li] + (np.arange(li.size) - np.repeat(np.cumsum(n) - n, n))
    Cu = 256 * k + 128
    Vc = _line_minor(Ua[li], Va[li], Ub[li], Vb[li], Cu)
    t = (Cu - Ua[li]).astype(np.float64) / (Ub[li] - Ua[li]).astype(np.float64)
    zf = (1.0 - t) * z[a[li]] + t * z[b[li]]
    key, keep = _depth_key(zf, draw[li])
    m0 = _floordiv(Vc, 256) - (width[li] - 1) // 2
    pix, keys = [], []
    for r in range(int(width.max()) if width.size else 0):
        m = m0 + r
        sel = keep & (r < width[li]) & (m >= 0) & (m < Wv[li])
        xm = xmaj[li][sel]
        i = np.where(xm, k[sel], m[sel])
        j = np.where(xm, m[sel], k[sel])
        pix.append(j * W + i)
        keys.append(key[sel])
    return np.concatenate(pix), np.concatenate(keys)


def _edges(X, Y, t0, t1, t2, Px, Py):
    X0, Y0, X1, Y1, X2, Y2 = X[t0], Y[t0], X[t1], Y[t1], X[t2], Y[t2]
    E0 = (X2 - X1) * (Py - Y1) - (Y2 - Y1) * (Px - X1)
    E1 = (X0 - X2) * (Py - Y2) - (Y0 - Y2) * (Px - X2)
    E2 = (X1 - X0) * (Py - Y0) - (Y1 - Y0) * (Px - X0)
    return E0, E1, E2


def _inside(E, dX, dY):
    return (E > 0) | ((E == 0) & ((dY < 0) | ((dY == 0) & (dX < 0))))


def _tri_bary(X, Y, t0, t1, t2, Px, Py):
    X0, Y0, X1, Y1, X2, Y2 = X[t0], Y[t0], X[t1], Y[t1], X[t2], Y[t2]
    A = (X1 - X0) * (Y2 - Y0) - (X2 - X0) * (Y1 - Y0)
    E0, E1, E2 = _edges(X, Y, t0, t1, t2, Px, Py)
    cov = _inside(E0, X2 - X1, Y2 - Y1) & _inside(E1, X0 - X2, Y0 - Y2) & _inside(E2, X1 - X0, Y1 - Y0)
    Af = A.astype(np.float64)
    return cov, E0.astype(np.float64) / Af, E1.astype(np.float64) / Af, E2.astype(np.float64) / Af


def _triangles(X, Y, z, cw, ok, f, draw, W, H, chunk=1 << 22):
    good = ok[f[:, 0]] & ok[f[:, 1]] & ok[f[:, 2]]
    Xf, Yf = X[f], Y[f]
    A = (Xf[:, 1] - Xf[:, 0]) * (Yf[:, 2] - Yf[:, 0]) - (Xf[:, 2] - Xf[:, 0]) * (Yf[:, 1] - Yf[:, 0])
    good &= A > 0
    i0 = np.maximum(_ceildiv(Xf.min(1) - 128, 256), 0)
    i1 = np.minimum(_floordiv(Xf.max(1) - 128, 256), W - 1)
    j0 = np.maximum(_ceildiv(Yf.min(1) - 128, 256), 0)
    j1 = np.minimum(_floordiv(Yf.max(1) - 128, 256), H - 1)
    bw, bh = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    n = np.where(good, bw * bh, 0)
    pix, keys = [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
    ids = np.nonzero(n)[0]
    cs = np.cumsum(n[ids])
    start = 0
    while start < ids.size:                                   # bounded memory: chunks of about `chunk` candidate pixels
        base = cs[start - 1] if start else 0
        stop = max(start + 1, int(np.searchsorted(cs, base + chunk, side="right")))
        sel = ids[start:stop]
        ti = np.repeat(sel, n[sel])
        r = np.arange(ti.size) - np.repeat(np.cumsum(n[sel]) - n[sel], n[sel])
        i = i0[ti] + r % bw[ti]
        j = j0[ti] + r // bw[ti]
        cov, b0, b1, b2 = _tri_bary(X, Y, f[ti, 0], f[ti, 1], f[ti, 2], 256 * i + 128, 256 * j + 128)
        zf = (b0 * z[f[ti, 0]] + b1 * z[f[ti, 1]]) + b2 * z[f[ti, 2]]
        key, keep = _depth_key(zf, draw[ti])
        keep &= cov
        pix.append((j * W + i)[keep])
        keys.append(key[keep])
        start = stop
    return np.concatenate(pix), np.concatenate(keys)


def _shade(pos, nrm, col, lit, ka, kd, light):
    """uint8 [n, 3] of interpolated attributes (float64 [n, 3] each)."""
    out = col.copy()
    if lit.any():
        L, amb, dif = light[0:3], light[3:6], light[6:9]
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        d = L[None, :] - pos
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        defined = (nn != 0) & (dd != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            sn, sl = np.sqrt(nn), np.sqrt(dd)
            nh = nrm / sn[:, None]
            lh = d / sl[:, None]
            cos = (nh[:, 0] * lh[:, 0] + nh[:, 1] * lh[:, 1]) + nh[:, 2] * lh[:, 2]
        cos = np.where(defined, np.maximum(cos, 0.0), 0.0)
        for c in range(3):
            light_c = ka * amb[c] + (kd * cos) * dif[c]
            out[:, c] = np.where(lit, light_c * col[:, c], col[:, c])
    return unorm8(out)


def _interp3(q, a):
    """((q0 a0 + q1 a1) + q2 a2) / ((q0 + q1) + q2) per component; q: list of 2 or 3 [n], a: list of [n, 3]."""
    if len(q) == 2:
        den = q[0] + q[1]
        return (q[0][:, None] * a[0] + q[1][:, None] * a[1]) / den[:, None]
    den = (q[0] + q[1]) + q[2]
    return ((q[0][:, None] * a[0] + q[1][:, None] * a[1]) + q[2][:, None] * a[2]) / den[:, None]


class _Prepared:
    """The selected models of one render, concatenated: what both backends read."""

    def __init__(self, models, mesh_indices):
        if not models:
            raise ValueError("render_views: no models")
        if len(models) > MAX_MODELS:
            raise ValueError(f"render_views: at most {MAX_MODELS} models, got {len(models)}")
        if mesh_indices is not None:
            bad = [i for i in mesh_indices if not (0 <= int(i) < len(models))]
            if bad:
                raise IndexError(f"render_views: mesh_indices {bad} out of range of {len(models)} models")
            chosen = {int(i) for i in mesh_indices}
        else:
            chosen = set(range(len(models)))
        self.sel = [i for i in range(len(models)) if i in chosen]      # list order, as the reference's loop
        pws, nws, cols, vbase = [], [], [], 0
        self.table = []    # per selected model: (kind, draw_base, n_prims, idx_offset, width, lit, ka, kd)
        idx, draw, ioff = [], 0, 0
        for i in self.sel:
            m = models[i]
            pw, nw, col = m.world()
            pws.append(pw)
            nws.append(nw)
            cols.append(col)
            ix = m.indices.astype(np.int64) + vbase
            idx.append(ix.reshape(-1))
            n = m.indices.shape[0]
            self.table.append((m.kind, draw, n, ioff, m.width, int(m.use_lighting), float(np.float32(m.ka)), float(np.float32(m.kd))))
            draw += n
            ioff += ix.size
            vbase += pw.shape[0]
        self.pw = np.concatenate(pws) if pws else np.zeros((0, 4))
        self.nw = np.concatenate(nws) if nws else np.zeros((0, 3))
        self.col = np.concatenate(cols) if cols else np.zeros((0, 3))
        self.idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        self.n_prims = draw
        if draw >= 1 << 32:
            raise ValueError("render_views: more than 2^32 primitives")


def _check_views(views, projections):
    views = np.asarray(views, dtype=np.float32).astype(np.float64)
    projections = np.asarray(projections, dtype=np.float32).astype(np.float64)
    if views.ndim == 2:
        views = views[None]
    if projections.ndim == 2:
        projections = projections[None]
    if views.shape[1:] != (4, 4) or projections.shape[1:] != (4, 4):
        raise ValueError("views and projections must be [V, 4, 4] (or one 4x4)")
    if projections.shape[0] == 1 and views.shape[0] > 1:
        projections = np.repeat(projections, views.shape[0], 0)
    if views.shape[0] != projections.shape[0] or views.shape[0] < 1:
        raise ValueError(f"{views.shape[0]} views but {projections.shape[0]} projections")
    return views, projections


def _render_cpu(prep, views, projs, W, H, light, bg):
    V = views.shape[0]
    img = np.empty((V, H, W, 3), np.uint8)
    dropped = 0
    for v in range(V):
        X, Y, z, cw, ok = _vertex_stage(prep.pw, views[v], projs[v], W, H)
        pix, keys = [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
        for kind, base, n, off, width, lit, ka, kd in prep.table:
            if n == 0:
                continue
            ix = prep.idx[off:off + kind * n].reshape(n, kind)
            draw = base + np.arange(n, dtype=np.int64)
            dropped += int((~ok[ix].all(1)).sum())
            if kind == 2:
                p, k = _lines(X, Y, z, cw, ok, ix[:, 0], ix[:, 1], draw, np.full(n, width, np.int64), W, H)
            else:
                p, k = _triangles(X, Y, z, cw, ok, ix, draw, W, H)
            pix.append(p)
            keys.append(k)
        buf = np.full(H * W, _NONE, np.uint64)
        np.minimum.at(buf, np.concatenate(pix), np.concatenate(keys))
        out = np.empty((H * W, 3), np.uint8)
        out[:] = bg
        hit = np.nonzero(buf != _NONE)[0]
        if hit.size:
            out[hit] = _resolve(prep, X, Y, z, cw, hit, (buf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64), W, light)
        img[v] = out.reshape(H, W, 3)[::-1]
    return img, dropped


def _resolve(prep, X, Y, z, cw, pix, draw, W, light):
    bases = np.array([t[1] for t in prep.table], np.int64)
    mi = np.searchsorted(bases, draw, side="right") - 1
    # (models without primitives share a base with the next one: searchsorted "right" picks the last, which owns the draw)
    res = np.empty((pix.size, 3), np.uint8)
    i, j = pix % W, pix // W
    for m, (kind, base, n, off, width, lit, ka, kd) in enumerate(prep.table):
        s = np.nonzero(mi == m)[0]
        if s.size == 0:
            continue
        p = draw[s] - base
        ix = prep.idx[off:off + kind * n].reshape(n, kind)[p]
        if kind == 2:
            a, b = ix[:, 0], ix[:, 1]
            xmaj = np.abs(X[b] - X[a]) >= np.abs(Y[b] - Y[a])
            Ua, Ub = np.where(xmaj, X[a], Y[a]), np.where(xmaj, X[b], Y[b])
            Cu = 256 * np.where(xmaj, i[s], j[s]) + 128
            t = (Cu - Ua).astype(np.float64) / (Ub - Ua).astype(np.float64)
            q = [(1.0 - t) / cw[a], t / cw[b]]
            vs = [a, b]
        else:
            _, b0, b1, b2 = _tri_bary(X, Y, ix[:, 0], ix[:, 1], ix[:, 2], 256 * i[s] + 128, 256 * j[s] + 128)
            q = [b0 * (1.0 / cw[ix[:, 0]]), b1 * (1.0 / cw[ix[:, 1]]), b2 * (1.0 / cw[ix[:, 2]])]
            vs = [ix[:, 0], ix[:, 1], ix[:, 2]]
        col = _interp3(q, [prep.col[x] for x in vs])
        if lit:
            pos = _interp3(q, [prep.pw[x, :3] for x in vs])
            nrm = _interp3(q, [prep.nw[x] for x in vs])
            res[s] = _shade(pos, nrm, col, np.ones(s.size, bool), ka, kd, light)
        else:
            res[s] = unorm8(col)
    return res


def gray_of(rgb):
    """OpenCV's 8-bit RGB2GRAY of uint8 [..., 3] (numpy)."""
    c = rgb.astype(np.int32)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def render_views(models, views, projections, width, height, lighting=None, mesh_indices=None, background=(0, 0, 0), device=None,
                 return_gray=False, _device_state=None):
    """Renders the selected models (all when mesh_indices is None) for every view: views [V, 4, 4] OpenGL view matrices and
    projections [V, 4, 4] (or one shared 4x4).  Returns (rgb uint8 [V, H, W, 3], dropped) -- plus gray uint8 [V, H, W] with
    return_gray -- as numpy arrays for device=None / "cpu", as device tensors for device="cuda".  `dropped` counts the dropped
    primitives over all views.  Raises before any launch on an empty model list or an out-of-range mesh index."""
    W, H = int(width), int(height)
    if W < 1 or H < 1 or W > (1 << 14) or H > (1 << 14):
        raise ValueError(f"render_views: bad size {W}x{H} (1 .. 16384)")
    prep = _Prepared(models, mesh_indices)
    vws, prj = _check_views(views, projections)
    light = (lighting.packed() if lighting is not None else np.zeros(9))
    bg = unorm8(np.asarray(background, np.float64)[:3])
    if device is None or str(device) == "cpu":
        img, dropped = _render_cpu(prep, vws, prj, W, H, light, bg)
        return (img, dropped, gray_of(img)) if return_gray else (img, dropped)
    from scene import _raster_device
    return _raster_device.render(prep, vws, prj, W, H, light, bg, device, return_gray, state=_device_state)
