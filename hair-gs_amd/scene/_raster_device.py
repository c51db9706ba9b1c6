"""Device path of scene/mesh_renderer.py: uploads the prepared models and runs csrc/hgs_raster.hip (vertex, count, scan, fill,
resolve).  One host read per render: the total length of the tile lists (with the dropped count)."""
import ctypes as C

import numpy as np


class DeviceMeshes:
    """The concatenated arrays of one model selection on the device (the reference's VBOs / EBOs): built once, reused by every
    render of the same selection."""

    def __init__(self, prep, device):
        import torch
        import hgs_runtime as rt
        self.device = torch.device(device)
        self.NV = int(prep.pw.shape[0])
        if self.NV >= 1 << 31:
            raise ValueError("render_views: more than 2^31 - 1 vertices")
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.pw, self.nw, self.col = up(prep.pw, np.float64), up(prep.nw, np.float64), up(prep.col, np.float64)
        self.idx = up(prep.idx.astype(np.uint32).view(np.int32), np.int32)
        tab = (rt.RasterModel * len(prep.table))()
        for k, (kind, base, n, off, width, lit, ka, kd) in enumerate(prep.table):
            tab[k] = rt.RasterModel(base, off, n, kind, width, lit, ka, kd)
        self.models = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
        self.n_models = len(prep.table)
        self.n_prims = int(prep.n_prims)


def render(prep, views, projs, W, H, light, bg, device, return_gray, state=None):
    import torch
    import hgs_runtime as rt
    L = rt.lib()
    dm = state if state is not None else DeviceMeshes(prep, device)
    dev = dm.device
    V = views.shape[0]
    if V > 65535:
        raise ValueError("render_views: at most 65535 views per call")
    T = int(L.hgs_raster_tiles(W, H))
    vw = torch.from_numpy(np.ascontiguousarray(views.reshape(V, 16))).to(dev)
    pj = torch.from_numpy(np.ascontiguousarray(projs.reshape(V, 16))).to(dev)
    vout = torch.empty(V * dm.NV * int(L.hgs_raster_vertex_bytes()), dtype=torch.uint8, device=dev)
    counts = torch.zeros(V * T, dtype=torch.int32, device=dev)
    dropped = torch.zeros(1, dtype=torch.int64, device=dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    gray = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if return_gray else None
    s = rt.current_stream()
    rt.check(L.hgs_raster_vertices(s, V, dm.NV, W, H, rt.ptr(dm.pw), rt.ptr(vw), rt.ptr(pj), rt.ptr(vout)))
    rt.check(L.hgs_raster_count(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), dm.NV, rt.ptr(vout),
                                rt.ptr(counts), rt.ptr(dropped)))
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = ends - counts
    total, n_dropped = torch.stack([ends[-1], dropped[0]]).tolist()       # the one host read
    lst = torch.empty(max(int(total), 1), dtype=torch.int32, device=dev)
    cursor = torch.zeros(V * T, dtype=torch.int32, device=dev)
    rt.check(L.hgs_raster_fill(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), dm.NV, rt.ptr(vout),
                               rt.ptr(counts), rt.ptr(offsets), rt.ptr(cursor), rt.ptr(lst)))
    lh = (C.c_double * 9)(*[float(x) for x in light])
    bh = (C.c_ubyte * 3)(*[int(x) for x in bg])
    rt.check(L.hgs_raster_resolve(s, V, W, H, dm.n_models, rt.ptr(dm.models), rt.ptr(dm.idx), dm.NV, rt.ptr(vout), rt.ptr(dm.pw),
                                  rt.ptr(dm.nw), rt.ptr(dm.col), lh, bh, rt.ptr(counts), rt.ptr(offsets), rt.ptr(lst), rt.ptr(rgb),
                                  rt.ptr(gray)))
    return (rgb, int(n_dropped), gray) if return_gray else (rgb, int(n_dropped))
