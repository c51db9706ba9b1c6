"""The 3-D direction term of a strand model: during Stage III every strand segment is pulled towards the hair line that the capture's
direction volume (utils/trace.py: init_cloud.py --directions lifts the lines, trace_strands.py --field [--fill N] writes the volume)
holds at the segment's midpoint.  The 2-D orientation term cannot tell a 3-D direction from its mirror about the view ray and is
silent where no view sees hair; the volume knows both.  train.py --lambda_direction L --direction_field PATH switches the term on;
the reference has no such term (loss/losses.py).

The contract (this module's numpy path, csrc/hgs_direction.hip and the loop restatement in tests/direction_reference.py state the same
thing).  All per-segment arithmetic is float32 with one rounding per operation, in exactly the order written (the kernel file is
built with -ffp-contract=off).  dot(p, q) = (p0*q0 + p1*q1) + p2*q2 throughout.

Volume.  A DirectionVolume is made from a utils.trace.Field (2 to 1024 nodes an axis, at most 2^26 in all: the field's own limits).
Its nodes are packed as vol float32 [nz, ny, nx, 4] = (dir.x, dir.y, dir.z, conf), so that one 16-byte load fetches a corner; a node
of which an entry is not finite in float32, or whose conf < 0, is stored as four zeros.  origin32 = float32(origin), inv_h32 =
float32(1/h) (the division in float64), as utils.head_sdf.HeadSDF forms them.  .on(device) keeps one device copy.

Per segment s of endpoint_pairs, for points P float32 [E, 3] and pairs [S, 2]:
    a = P[pairs[s][0]], b = P[pairs[s][1]];  u = b - a;  m = (a + b) * 0.5f;  uu = dot(u, u)
    t = (m - origin) * inv_h per axis;  ok = every t finite and 0 <= t < n_axis - 1   (the range test precedes every load)
    i = floor(t), f = t - i;  g0 = 1 - f, g1 = f
    w = 0, v = 0;  corners z outermost, then y, then x, each 0 then 1:
        tw = (gx*gy)*gz;  c = vol[corner];  q = tw*c.w;  w = w + q
        if dot(c.xyz, u) < 0: q = -q
        v_j = v_j + q*c_j
    nn = dot(v, v)
    active = ok and w >= min_conf and nn finite and > 0 and uu finite and > 0
    fd = v / sqrt(nn)  (three divisions);  cu = dot(u, fd);  k = cu / uu
    term_s = 1 - cu*k                      (= sin^2 of the angle between the segment and the field's line)
    gs_s   = (-2*k) * (fd - k*u)           (d term / d u; the sampled line is a constant: no gradient through m)
An inactive segment gives term = 0, gs = 0 (and w = 0 where it is out of range).  The corner loop and the sign rule are the tracer's
(utils/trace.py, Trace) with the segment in the place of the previous direction: negating any node directions changes no bit, apart
from dot == 0 exactly.

Value.  L = float32((sum_s term_s in float64) / S) over ALL S segments -- the head term's convention: a segment's pull does not change
when another segment gates in or out; L = 0 for S = 0.  The kernel and the numpy path differ in the order of the float64 sum only.

Gradient.  Through an incidence table: for endpoint e the entries (s, side) with pairs[s][side] == e, ascending by (s, side), as CSR
offsets int32 [E + 1] and entries int32 [2S] holding 2*s + side.
    acc = 0.0f;  for each entry in order:  acc_j = acc_j + (side ? gs[s][j] : -gs[s][j])
    d_P[e][j] = acc_j * (upstream / float32(S))          (one float32 division, one multiplication; 0 for S = 0)
The table allows any degree: a junction of three segments is summed the same way; an endpoint that no segment uses gets 0.  pairs
entries outside [0, E) are refused when the table is built; the kernels trust the table.

Known limits.  Every row of endpoint_pairs takes part, background segments included: where the volume has no data they are inactive.
The gate (range, min_conf) is a step function of position.  There is no gradient through the lookup position: the term turns a
segment, it does not move it to where the field agrees with it.  min_conf and the weight are knobs, not measured optima.  The volume
is the capture's, not the model's: building it from the trained strands, and a per-segment foreground weight, are later work.

The functions below are the numpy path; hgs_runtime.fused.direction_loss is the device op, loss.losses.strand_direction_loss the same
statement in torch ops.  Neither falls back to the other."""
import numpy as np

from utils.trace import Field, load_field

MAX_SEGMENTS = 1 << 28


class DirectionVolume:
    """origin f64 [3], spacing, shape (nx, ny, nz) of a utils.trace.Field and its nodes packed as vol float32 [nz, ny, nx, 4] =
    (dir.x, dir.y, dir.z, conf); origin32, inv_h32: the float32 constants of the term.  The device copies are cached on the object."""

    def __init__(self, field):
        if not isinstance(field, Field):
            raise ValueError(f"a utils.trace.Field expected, not {type(field).__name__}")
        self.origin, self.spacing, self.shape = field.origin, float(field.spacing), field.shape
        with np.errstate(all="ignore"):
            vol = np.concatenate([field.dir, field.conf[..., None]], axis=-1).astype(np.float32)
            bad = ~np.isfinite(vol).all(axis=-1) | (vol[..., 3] < 0)
        vol[bad] = 0
        self.vol = np.ascontiguousarray(vol)
        self.cleared = int(bad.sum())
        self.origin32 = self.origin.astype(np.float32)
        self.inv_h32 = np.float32(1.0 / self.spacing)
        if not (np.isfinite(self.origin32).all() and np.isfinite(self.inv_h32) and self.inv_h32 > 0):
            raise ValueError("origin and 1/spacing must be finite in float32")
        self._dev = {}

    @classmethod
    def load(cls, path):
        """The DirectionVolume of an .npz that trace_strands.py --field wrote; ValueError, in this module's words, for anything else."""
        try:
            return cls(load_field(path))
        except (OSError, EOFError, KeyError) as e:
            raise ValueError(f"{path}: not a direction volume ({e})") from None
        except ValueError as e:
            if str(e).startswith(str(path)):
                raise
            raise ValueError(f"{path}: not a direction volume ({e})") from None

    def on(self, device):
        """{"vol": float32 [nodes, 4], "origin", "inv_h", "top": float32 constants of the torch statement} on `device`, made once."""
        import torch
        device = torch.device(device)
        key = str(device if device.index is not None or device.type != "cuda" else torch.device("cuda", torch.cuda.current_device()))
        hit = self._dev.get(key)
        if hit is None:
            nx, ny, nz = self.shape
            hit = self._dev[key] = dict(
                vol=torch.from_numpy(self.vol.reshape(-1, 4)).to(device),
                origin=torch.from_numpy(self.origin32.copy()).to(device),
                inv_h=torch.tensor(float(self.inv_h32), dtype=torch.float32, device=device),
                top=torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=device))
        return hit


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def check_pairs(pairs, E):
    """pairs as int64 [S, 2] with every entry in [0, E); ValueError otherwise."""
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError(f"pairs of shape {pairs.shape} ({pairs.dtype}): integers [S, 2] expected")
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    if pairs.shape[0] > MAX_SEGMENTS:
        raise ValueError(f"{pairs.shape[0]} segments (at most 2^28)")
    if pairs.size and (pairs.min() < 0 or pairs.max() >= E):
        raise ValueError(f"pairs holds endpoint ids from {int(pairs.min())} to {int(pairs.max())}, the model has {E} endpoints")
    return pairs


def _points32(points):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points of shape {points.shape}: [E, 3] expected")
    return np.ascontiguousarray(points, dtype=np.float32)


def segments(points, pairs, volume, min_conf):
    """(term f32 [S], w f32 [S], gs f32 [S, 3], active bool [S]) of the contract's per-segment statement."""
    P = _points32(points)
    pairs = check_pairs(pairs, P.shape[0])
    nx, ny, nz = volume.shape
    vol = volume.vol.reshape(-1, 4)
    min_conf, half, one, zero = np.float32(min_conf), np.float32(0.5), np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        a, b = P[pairs[:, 0]], P[pairs[:, 1]]
        u = [b[:, j] - a[:, j] for j in range(3)]
        m = np.stack([(a[:, j] + b[:, j]) * half for j in range(3)], axis=1)
        uu = _dot(u, u)
        t = (m - volume.origin32[None, :]) * volume.inv_h32
        top = np.array([nx - 1, ny - 1, nz - 1], np.float32)
        ok = (np.isfinite(t) & (t >= 0) & (t < top[None, :])).all(axis=1)
        t = np.where(ok[:, None], t, zero)                                      # (rows out of range: any valid address)
        fl = np.floor(t)
        i = fl.astype(np.int64)
        f = t - fl
        g = (one - f, f)
        w = np.zeros(pairs.shape[0], np.float32)
        v = [np.zeros(pairs.shape[0], np.float32) for _ in range(3)]
        for z in (0, 1):
            for y in (0, 1):
                for x in (0, 1):
                    tw = (g[x][:, 0] * g[y][:, 1]) * g[z][:, 2]
                    c = vol[((i[:, 2] + z) * ny + (i[:, 1] + y)) * nx + (i[:, 0] + x)]
                    q = tw * c[:, 3]
                    w = w + q
                    q = np.where(_dot((c[:, 0], c[:, 1], c[:, 2]), u) < 0, -q, q)
                    v = [v[j] + q * c[:, j] for j in range(3)]
        nn = _dot(v, v)
        active = ok & (w >= min_conf) & np.isfinite(nn) & (nn > 0) & np.isfinite(uu) & (uu > 0)
        ln = np.sqrt(nn)
        fd = [v[j] / ln for j in range(3)]
        cu = _dot(u, fd)
        k = cu / uu
        term = np.where(active, one - cu * k, zero)
        m2 = np.float32(-2.0) * k
        gs = np.stack([np.where(active, m2 * (fd[j] - k * u[j]), zero) for j in range(3)], axis=1)
        w = np.where(ok, w, zero)
    assert term.dtype == np.float32 and w.dtype == np.float32 and gs.dtype == np.float32
    return term, w, gs, active


def incidence(pairs, E):
    """(offsets int32 [E + 1], entries int32 [2S]) of the contract's table: endpoint e owns entries[offsets[e]:offsets[e + 1]], the
    values 2*s + side with pairs[s][side] == e, ascending."""
    pairs = check_pairs(pairs, int(E))
    flat = pairs.reshape(-1)
    entries = np.argsort(flat, kind="stable").astype(np.int32)
    offsets = np.zeros(int(E) + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=int(E)), out=offsets[1:])
    return offsets.astype(np.int32), entries


def gather(gs, offsets, entries, S, upstream=1.0):
    """d_P f32 [E, 3] of the contract's gradient statement for per-segment gs f32 [S, 3]."""
    gs = np.ascontiguousarray(gs, dtype=np.float32)
    E = offsets.shape[0] - 1
    deg = (offsets[1:] - offsets[:-1]).astype(np.int64)
    acc = np.zeros((E, 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(int(deg.max()) if E else 0):
            e = np.nonzero(deg > r)[0]
            ent = entries[offsets[e].astype(np.int64) + r].astype(np.int64)
            row = gs[ent >> 1]
            acc[e] = acc[e] + np.where((ent & 1)[:, None] == 1, row, -row)
        scale = np.float32(upstream) / np.float32(S) if S > 0 else np.float32(0)
        d = acc * scale
    assert d.dtype == np.float32
    return d


def loss(points, pairs, volume, min_conf, upstream=1.0, info=None):
    """(L float32, dL/dpoints f32 [E, 3]) of the contract's term for an upstream gradient.  `info`, a dict, receives "term", "w", "gs",
    "active" (the count)."""
    P = _points32(points)
    pairs = check_pairs(pairs, P.shape[0])
    term, w, gs, active = segments(P, pairs, volume, min_conf)
    S = pairs.shape[0]
    offsets, entries = incidence(pairs, P.shape[0])
    L = np.float32(term.astype(np.float64).sum() / np.float64(S)) if S else np.float32(0)
    if info is not None:
        info.update(term=term, w=w, gs=gs, active=int(active.sum()))
    return L, gather(gs, offsets, entries, S, upstream)
