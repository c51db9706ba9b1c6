"""The rasterizer of the dataset synthesis on the GPU (csrc/hgs_raster.hip) against the brute force of
tests/mesh_raster_reference.py on the hard cases of tests/mesh_raster_cases.py.  Every comparison is exact and nothing is exempt:
the whole path through render_views(device="cuda"); each stage through the C ABI (vertex records bit for bit, per-tile counts,
per-tile lists as sets with every entry once, resolved bytes), with every output inside a larger allocation whose guard bytes must
survive; the tile lists permuted on the device before the resolve; and repeated runs, a side stream and a reused device state."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.mesh_raster_cases import CASES, expected
from tests.mesh_raster_reference import INT_MIN, reference

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
RECORD = np.dtype([("z", "<f8"), ("w", "<f8"), ("X", "<i4"), ("Y", "<i4")])


class Guarded:
    """n bytes of device memory inside a larger allocation of the fill pattern; zero=True clears the n bytes (accumulators)."""

    def __init__(self, n, zero=False):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.uint8, device="cuda")
        if zero:
            self.buf[GUARD:GUARD + self.n] = 0
        self.ptr = self.buf.data_ptr() + GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def numpy(self, dtype):
        return self.body().cpu().numpy().view(dtype)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())


def _render(name, **kw):
    from scene.mesh_renderer import render_views
    models, views, projs, W, H, light, bg, sel = CASES[name]()
    img, dropped, gray = render_views(models, views, projs, W, H, light, mesh_indices=sel, background=bg, return_gray=True,
                                      device="cuda", **kw)
    return img.cpu().numpy(), dropped, gray.cpu().numpy()


def _same_bytes(name, img, ref_rgb, what):
    bad = (img != ref_rgb).any(-1)
    assert not bad.any(), f"{name} {what}: {int(bad.sum())} pixel(s) differ, first (view, image row, column) {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("name", list(CASES))
def test_render_views_equals_reference(name):
    ref = expected(name)
    img, dropped, gray = _render(name)
    assert img.shape == ref.rgb.shape and dropped == ref.dropped
    _same_bytes(name, img, ref.rgb, "rgb")
    assert np.array_equal(gray, ref.gray)


def _stages(name, permute_seed=None):
    """The launches of scene/_raster_device.render through the C ABI, each stage checked against the reference as it ends."""
    import hgs_runtime as rt
    from scene import mesh_renderer as R
    from scene._raster_device import DeviceMeshes
    L = rt.lib()
    ref = expected(name)
    models, views, projs, W, H, lighting, bg, sel = CASES[name]()
    prep = R._Prepared(models, sel)
    vws, prj = R._check_views(views, projs)
    light = lighting.packed() if lighting is not None else np.zeros(9)
    bgb = R.unorm8(np.asarray(bg, np.float64)[:3])
    dm = DeviceMeshes(prep, "cuda")
    V, NV, T = vws.shape[0], dm.NV, int(L.hgs_raster_tiles(W, H))
    assert (V, NV, T, dm.n_prims) == (ref.V, ref.NV, ref.TX * ref.TY, ref.n_prims)
    assert int(L.hgs_raster_vertex_bytes()) == RECORD.itemsize
    vw = torch.from_numpy(np.ascontiguousarray(vws.reshape(V, 16))).cuda()
    pj = torch.from_numpy(np.ascontiguousarray(prj.reshape(V, 16))).cuda()
    s = rt.current_stream()
    bufs = {}

    # vertices
    vout = bufs["vertices"] = Guarded(V * NV * RECORD.itemsize)
    rt.check(L.hgs_raster_vertices(s, V, NV, W, H, rt.ptr(dm.pw), rt.ptr(vw), rt.ptr(pj), vout.ptr))
    got = vout.numpy(RECORD).reshape(V, NV)
    for v in range(V):
        z, w, X, Y = ref.vertices[v]
        assert np.array_equal(got[v]["X"], X) and np.array_equal(got[v]["Y"], Y), f"{name} view {v}: snapped coordinates"
        assert np.array_equal(got[v]["X"] == INT_MIN, X == INT_MIN)
        assert np.array_equal(got[v]["z"].view(np.uint64), z.view(np.uint64)), f"{name} view {v}: z_w bits"
        assert np.array_equal(got[v]["w"].view(np.uint64), w.view(np.uint64)), f"{name} view {v}: c.w bits"

    # count
    counts = bufs["counts"] = Guarded(V * T * 4, zero=True)
    dropped = bufs["dropped"] = Guarded(8, zero=True)
    rt.check(L.hgs_raster_count(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), NV, vout.ptr, counts.ptr,
                                dropped.ptr))
    want_counts = np.array([[len(t) for t in ref.tiles[v]] for v in range(V)], np.int32)
    got_counts = counts.numpy(np.int32).reshape(V, T)
    wrong = np.argwhere(got_counts != want_counts)
    assert wrong.size == 0, f"{name}: tile counts differ at (view, tile) {wrong[:5].tolist()}"
    assert int(dropped.numpy(np.uint64)[0]) == ref.dropped

    # scan (the caller's), fill
    cnt = counts.body().view(torch.int32)
    ends = torch.cumsum(cnt, 0, dtype=torch.int64)
    offsets = ends - cnt
    total = int(ends[-1])
    lst = bufs["list"] = Guarded(max(total, 1) * 4)
    cursor = bufs["cursor"] = Guarded(V * T * 4, zero=True)
    rt.check(L.hgs_raster_fill(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), NV, vout.ptr, counts.ptr,
                               rt.ptr(offsets), cursor.ptr, lst.ptr))
    assert np.array_equal(cursor.numpy(np.int32).reshape(V, T), want_counts), f"{name}: cursors differ from the counts"
    flat = lst.numpy(np.uint32)
    off = offsets.cpu().numpy().reshape(V, T)
    for v in range(V):
        for t in range(T):
            seg = flat[off[v, t]:off[v, t] + want_counts[v, t]].tolist()
            assert sorted(seg) == sorted(ref.tiles[v][t]), f"{name}: list of view {v} tile {t}"       # (a set: every entry once)
    if total == 0:
        assert (flat.view(np.uint8) == FILL).all()
    assert np.array_equal(counts.numpy(np.int32).reshape(V, T), want_counts)                        # fill leaves the counts alone

    if permute_seed is not None and total > 0:
        rng = np.random.default_rng(permute_seed)
        src = np.arange(total)
        for o, n in zip(off.reshape(-1), want_counts.reshape(-1)):
            src[o:o + n] = o + rng.permutation(n)
        words = lst.body().view(torch.int32)
        words.copy_(words[torch.from_numpy(src).cuda()])

    # resolve
    rgb = bufs["rgb"] = Guarded(V * H * W * 3)
    gray = bufs["gray"] = Guarded(V * H * W)
    lh = (C.c_double * 9)(*[float(x) for x in light])
    bh = (C.c_ubyte * 3)(*[int(x) for x in bgb])
    rt.check(L.hgs_raster_resolve(s, V, W, H, dm.n_models, rt.ptr(dm.models), rt.ptr(dm.idx), NV, vout.ptr, rt.ptr(dm.pw), rt.ptr(dm.nw),
                                  rt.ptr(dm.col), lh, bh, counts.ptr, rt.ptr(offsets), lst.ptr, rgb.ptr, gray.ptr))
    img = rgb.numpy(np.uint8).reshape(V, H, W, 3)
    _same_bytes(name, img, ref.rgb, "resolve")
    assert np.array_equal(gray.numpy(np.uint8).reshape(V, H, W), ref.gray)
    for k, b in bufs.items():
        assert b.guards_intact(), f"{name}: bytes written outside the {k} buffer"
    assert np.array_equal(vout.numpy(RECORD).reshape(V, NV), got)                                    # inputs of later stages unchanged
    return img


@pytest.mark.parametrize("name", list(CASES))
def test_stages_equal_reference(name):
    _stages(name)


@pytest.mark.parametrize("name", list(CASES))
def test_list_order_does_not_matter(name):
    _stages(name, permute_seed=7)


@pytest.mark.parametrize("name", list(CASES))
def test_reproducible_and_on_a_side_stream(name):
    first, second = _render(name), _render(name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _render(name)
    side.synchronize()
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and first[1] == other[1] and np.array_equal(first[2], other[2])
    _same_bytes(name, third[0], expected(name).rgb, "side stream")


@pytest.mark.parametrize("name", ["views_3", "dropped_rules", "shading_persp"])
def test_reused_device_state(name):
    """One DeviceMeshes used for two different view sets gives the bytes of fresh states."""
    from scene import mesh_renderer as R
    from scene._raster_device import DeviceMeshes
    models, views, projs, W, H, light, bg, sel = CASES[name]()
    views, projs = R._check_views(views, projs)
    V = views.shape[0]
    if V == 1:                                                   # a second view set: the camera moved and the image mirrored
        v2 = views.copy()
        v2[0, :3, 3] += [0.03125, -0.015625, -0.0625]
        sets = [(views, projs), (v2, projs * np.array([-1.0, 1.0, 1.0, 1.0])[None, :, None])]
    else:
        sets = [(views[:2], projs[:2]), (views[::-1].copy(), projs[::-1].copy())]
    state = DeviceMeshes(R._Prepared(models, sel), "cuda")
    kw = dict(mesh_indices=sel, background=bg, return_gray=True, device="cuda")
    for vs, ps in sets + sets[:1]:
        a = R.render_views(models, vs, ps, W, H, light, _device_state=state, **kw)
        b = R.render_views(models, vs, ps, W, H, light, **kw)
        c = reference(models, vs, ps, W, H, light, bg, sel)
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])
        assert np.array_equal(a[0].cpu().numpy(), c.rgb) and a[1] == c.dropped and np.array_equal(a[2].cpu().numpy(), c.gray)
    assert not torch.equal(R.render_views(models, *sets[0], W, H, light, _device_state=state, **kw)[0][0],
                           R.render_views(models, *sets[1], W, H, light, _device_state=state, **kw)[0][0])
