"""Fields, volumes, strands and knobs of the root attachment's tests (tests/test_attach_cpu.py, tests/test_attach_gpu.py): the smallest
at which hgs_root_attach / hgs_strand_rejoin (csrc/hgs_attach.hip) and the numpy path of scene/strand_attach.py can go wrong.  A case is
a dict: points float32 [P, 3], attrs float32 [P, C], offsets int64 [K + 1], field (a name of collide_cases.field, or "plateau"),
volume (a name of volume(), or None) and knobs (the keyword arguments of the march)."""
import functools

import numpy as np

from tests import collide_cases as CC

KS = CC.KS                                       # strand counts: around a wave and a workgroup of 256, and several workgroups
MS = (0, 2, 3, 100)                              # points per resampled strand; 0: the joined joints


# ---- fields and volumes ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field(name):
    """collide_cases' fields, and "plateau": its flat field raised by one, so that the cell [1, 2]^3 (and [0, 1] x [1, 2]^2) of zero
    gradient lies 0.75 ABOVE the surface -- a root there is not already rooted and has no way down."""
    if name == "plateau":
        from utils.head_sdf import HeadSDF
        flat = CC.field("flat")
        return HeadSDF(flat.origin, flat.spacing, flat.shape, flat.phi + np.float32(1.0))
    return CC.field(name)


@functools.lru_cache(maxsize=None)
def volume(name):
    """7^3 nodes from -1.8 by 0.6 (roots beyond 1.8 on an axis are out of its range).  "swirl": directions around the z axis leaning
    outward, conf uniform in [0, 1.5) (so min_conf decides); "const": one direction everywhere, conf 1; "zero": swirl with conf 0
    everywhere; "flip": swirl with about half of its dir entries negated."""
    from utils.trace import Field
    rng = np.random.default_rng(11)
    g, o, h = 7, -1.8, 0.6
    ax = o + h * np.arange(g)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    pos = np.stack([x, y, z], axis=-1)
    d = np.cross(np.array([0.0, 0.0, 1.0]), pos) + 0.3 * pos
    ln = np.linalg.norm(d, axis=-1, keepdims=True)
    d = np.where(ln > 0, d / np.where(ln > 0, ln, 1.0), np.array([1.0, 0.0, 0.0]))
    conf = rng.uniform(0.0, 1.5, size=(g, g, g))
    flip = rng.random((g, g, g)) < 0.5
    if name == "const":
        c = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
        d, conf = np.broadcast_to(c, d.shape).copy(), np.ones((g, g, g))
    elif name == "zero":
        conf = np.zeros((g, g, g))
    elif name == "flip":
        d = np.where(flip[..., None], -d, d)
    elif name != "swirl":
        raise KeyError(name)
    return Field(np.array([o, o, o]), h, (g, g, g), d, conf)


# ---- strands -----------------------------------------------------------------------------------------------------------------------
def _with_attrs(points, offsets, C=3, seed=0):
    attrs = np.random.default_rng(seed).uniform(-1.0, 2.0, size=(points.shape[0], C)).astype(np.float32)
    return points, attrs, offsets


def _flip_point(sdf, predicate, lo, hi, y=0.2, z=0.1):
    """The two neighbouring float32 x between lo and hi (predicate true at lo, false at hi, on the line y, z) where it changes."""
    from utils.head_sdf import trilinear

    def holds(x):
        ok, d, _, _, _ = trilinear(np.array([[x, y, z]], np.float32), sdf)
        return bool(ok[0]) and bool(predicate(np.float64(d[0])))

    lo, hi = np.float32(lo), np.float32(hi)
    assert holds(lo) and not holds(hi)
    while np.nextafter(lo, hi) != hi:
        mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
        lo, hi = (mid, hi) if holds(mid) else (lo, mid)
    return float(lo), float(hi)


def special_strands(fname, margin, max_distance):
    """On a sphere field of radius 1 in the box [-2, 2]^3: the roots that take every branch of the contract's head.  Returns (the
    strands, index by name)."""
    nan, inf = np.nan, np.inf
    sdf = field(fname)
    m, tl = np.float64(np.float32(margin)), np.float64(np.float32(1e-3 * sdf.spacing))
    near_in, near_out = _flip_point(sdf, lambda d: d <= m + tl, 0.5, 1.5)
    far_in, far_out = _flip_point(sdf, lambda d: not d - m > max_distance, 1.0, 1.9)
    s = dict(
        empty=np.zeros((0, 3)), one=np.array([[1.3, 0.1, 0.0]]), one_nan=np.array([[nan, 0.0, 0.0]]),
        two=np.array([[1.3, 0.2, -0.1], [1.5, 0.4, -0.2]]),
        near_last=np.array([[near_in, 0.2, 0.1], [1.4, 0.3, 0.1]]),              # the last float32 that is already rooted
        near_first=np.array([[near_out, 0.2, 0.1], [1.4, 0.3, 0.1]]),            # the first that is not: lands without a step
        inside=np.array([[0.4, 0.3, 0.2], [0.9, 0.8, 0.5], [1.3, 1.0, 0.6]]),     # a root inside the head: already rooted
        centre=np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]),
        outside=np.array([[5.0, 5.0, 5.0], [5.5, 5.0, 5.0]]),                     # out of the field's range
        at_top=np.array([[2.0, 0.0, 0.0], [2.5, 0.0, 0.0]]),                      # t == n - 1: out of range
        below=np.array([[-2.001, 0.0, 0.0], [-2.5, 0.0, 0.0]]),
        nan_root=np.array([[nan, 0.2, 0.1], [1.4, 0.3, 0.1]]), inf_root=np.array([[1.2, inf, 0.1], [1.4, 0.3, 0.1]]),
        ninf_root=np.array([[1.2, 0.2, -inf], [1.4, 0.3, 0.1]]), huge_root=np.array([[3e38, 0.0, 0.0], [1.4, 0.3, 0.1]]),
        nan_second=np.array([[1.3, 0.2, 0.1], [nan, 0.3, 0.1], [1.6, 0.4, 0.1]]),  # no tangent: starts down the gradient
        inf_second=np.array([[1.3, -0.2, 0.1], [inf, 0.3, 0.1]]),
        doubled=np.array([[1.25, 0.3, -0.4], [1.25, 0.3, -0.4], [1.5, 0.4, -0.5]]),   # p_0 == p_1
        far_last=np.array([[far_in, 0.2, 0.1], [1.95, 0.3, 0.1]]),               # the last float32 within max_distance
        far_first=np.array([[far_out, 0.2, 0.1], [1.95, 0.3, 0.1]]),             # just beyond it
        away=np.array([[1.4, 0.0, 0.0], [1.1, 0.0, 0.0], [0.9, 0.1, 0.0]]),        # the backward tangent points away from the head
        sideways=np.array([[0.0, 1.35, 0.3], [-0.6, 1.35, 0.2], [-1.0, 1.3, 0.1]]),  # ... along the surface
        inward=np.array([[-0.8, -0.8, 0.7], [-1.2, -1.2, 1.0]]),                  # ... straight at it
        corner=np.array([[1.9, 1.9, 1.9], [1.95, 1.95, 1.95]]),                   # the far corner of the box, outside the volume
        long=np.array([[0.3, -1.7, 0.2], [0.3, -1.9, 0.3], [0.2, -1.95, 0.5], [0.1, -1.9, 0.8], [0.0, -1.8, 1.0]]),
    )
    names = tuple(s)
    pts, off = CC._pack([s[k] for k in names])
    return _with_attrs(pts, off, C=3, seed=1), {k: i for i, k in enumerate(names)}


@functools.lru_cache(maxsize=None)
def sphere_strands(K=1000, seed=5, joints=None):
    """K strands rooted at radius 1.03 to 1.6 around the unit sphere, the tangent tilted either way.
    joints=None: ragged, 2 to 6 joints, with a strand of 0 or 1 joints in about one of eight.  The first k strands are the case of k."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        t = np.cross(nrm, rng.normal(size=3))
        t /= np.linalg.norm(t)
        d = t + rng.uniform(-0.8, 0.8) * nrm
        d /= np.linalg.norm(d)
        n = joints if joints is not None else (int(rng.integers(0, 2)) if rng.random() < 0.125 else int(rng.integers(2, 7)))
        s = np.linspace(0.0, 0.5, max(n, 1))[:n, None]
        out.append(rng.uniform(1.03, 1.6) * nrm[None, :] + s * d[None, :] + 0.01 * rng.normal(size=(n, 3)) if n else np.zeros((0, 3)))
    pts, off = CC._pack(out)
    return _with_attrs(pts, off, C=5, seed=seed + 1)


def first_strands(points, attrs, offsets, K):
    return points[:offsets[K]], attrs[:offsets[K]], offsets[:K + 1]


def _case(strands, fname, vname=None, **knobs):
    pts, attrs, off = strands
    return dict(points=pts, attrs=attrs, offsets=off, field=fname, volume=vname, knobs=knobs)


def steps_strand():
    """A root far out on the diagonal of sphere24's box, and the number of loop passes its march takes (the steps and the landing):
    with max_steps equal to that it arrives, with one fewer it does not.  The restatement counts."""
    from tests import attach_reference as AR
    pts, off = CC._pack([np.array([[1.0, 1.05, 0.95], [1.1, 1.2, 1.0]])])
    _, count, reason, _ = AR.march(pts, off, field("sphere24"), None, max_steps=64)
    assert reason[0] == AR.REACHED
    return _with_attrs(pts, off, C=1, seed=2), int(count[0])


@functools.lru_cache(maxsize=None)
def hard_cases():
    """name -> case."""
    cases = {}
    for fname, margin, vname, extra in (("sphere9", 0.0, None, {}), ("sphere9", 0.05, "swirl", {}), ("sphere24", 0.02, "swirl", dict(pull=0.5)),
                                        ("sphere24", 0.0, "const", dict(pull=0.0, descent=0.5)), ("sphere9", 0.0, "zero", dict(pull=4.0)),
                                        ("sphere24", 0.02, "flip", dict(pull=0.5, min_conf=0.2, land_iters=1)),
                                        ("sphere24", 0.02, "swirl", dict(pull=0.5, min_conf=0.2, land_iters=1)),
                                        ("sphere24", 0.0, None, dict(tol=0.0, land_iters=8, step=0.05, descent=1.0))):
        (strands, _) = special_strands(fname, margin, 0.45)
        tag = "_".join(f"{k}{v}" for k, v in extra.items())
        cases[f"special_{fname}_m{margin}_{vname}" + ("_" + tag if tag else "")] = _case(strands, fname, vname, margin=margin, max_distance=0.45, **extra)
    sp = sphere_strands()
    few = first_strands(*sp, 120)
    cases["scene_plain"] = _case(few, "sphere9")
    cases["scene_swirl"] = _case(few, "sphere24", "swirl", margin=0.02, pull=0.5)
    cases["scene_flip"] = _case(few, "sphere24", "flip", margin=0.02, pull=0.5)
    cases["scene_small_steps"] = _case(few, "sphere24", "const", step=0.03, max_steps=12, pull=0.25)      # most run out of steps
    cases["scene_one_step"] = _case(few, "sphere9", "swirl", max_steps=1)
    st, passes = steps_strand()
    cases["steps_exact"] = _case(st, "sphere24", max_steps=passes)
    cases["steps_one_short"] = _case(st, "sphere24", max_steps=passes - 1)
    # the plateau has no surface: roots in a cell of zero gradient stop at once, those on the slope march down it into one.  On
    # collide_cases' flat field itself the zero-gradient cells lie at -0.25, so a root there is already rooted (d <= margin + tol)
    flat = CC._pack([np.array([[1.5, 1.5, 1.5], [1.6, 1.5, 1.5]]), np.array([[2.9, 1.5, 1.5], [3.0, 1.6, 1.5]]),
                     np.array([[2.9, 0.5, 0.5], [3.0, 0.5, 0.6]]), np.array([[0.5, 1.25, 1.75], [0.5, 1.0, 2.0]])])
    cases["plateau"] = _case(_with_attrs(*flat, C=2, seed=3), "plateau", step=0.4)
    cases["flat"] = _case(_with_attrs(*flat, C=2, seed=3), "flat", step=0.4)
    # one cell: a march that leaves it sideways, one that lands in it, one rooted outside it
    tiny = CC._pack([np.array([[0.9, 0.9, 0.5], [1.05, 0.645, 0.5]]), np.array([[0.9, 0.4, 0.5], [0.95, 0.4, 0.5]]),
                     np.array([[0.95, 0.5, 1.0], [0.95, 0.5, 1.5]])])
    cases["tiny"] = _case(_with_attrs(*tiny, C=2, seed=4), "tiny", step=0.2, pull=0.0)
    slab = CC.box_strands(CC.slab_field(), 60, 3, 5)
    cases["slab"] = _case(_with_attrs(*slab, C=4, seed=6), "slab")
    cases["slab_margin"] = _case(_with_attrs(*slab, C=4, seed=6), "slab", margin=0.04, pull=2.0, step=0.05)
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(1, np.int64))
    cases["no_strands"] = _case(none, "sphere9")
    cases["empty_strands_only"] = _case((none[0], np.zeros((0, 0), np.float32), np.zeros(4, np.int64)), "sphere9", "swirl")
    return cases


HARD_NAMES = ("special_sphere9_m0.0_None", "special_sphere9_m0.05_swirl", "special_sphere24_m0.02_swirl_pull0.5",
              "special_sphere24_m0.0_const_pull0.0_descent0.5", "special_sphere9_m0.0_zero_pull4.0",
              "special_sphere24_m0.02_flip_pull0.5_min_conf0.2_land_iters1", "special_sphere24_m0.02_swirl_pull0.5_min_conf0.2_land_iters1",
              "special_sphere24_m0.0_None_tol0.0_land_iters8_step0.05_descent1.0", "scene_plain", "scene_swirl", "scene_flip",
              "scene_small_steps", "scene_one_step", "steps_exact", "steps_one_short", "plateau", "flat", "tiny", "slab", "slab_margin",
              "no_strands", "empty_strands_only")
COUNTED = dict(field="sphere9", volume="swirl", knobs=dict(margin=0.03, pull=0.5))     # the strand-count cases: sphere_strands()[:K]

# ---- the analytic head: every strand must arrive -------------------------------------------------------------------------------------
LANDING_GRIDS = (9, 24)
LANDING_MARGINS = (0.0, 0.02)
LANDING_PULLS = (0.0, 0.5, 1.0, 4.0)


def landing_strands():
    """300 strands of 3 joints, rooted at radius 1.03 to 1.6."""
    return sphere_strands(K=300, seed=9, joints=3)
