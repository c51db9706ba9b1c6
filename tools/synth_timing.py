#!/usr/bin/env python3
"""Times the dataset synthesis renderer (scene/mesh_renderer.py, csrc/hgs_raster.hip): a 16-view batch at 1000x1000 of 10^4
strands x 100 vertices (synthetic.strand_polylines, about 10^6 segments) around a sphere head of about 2 x 10^4 triangles, the
image render ([lit head, hair]) plus the mask render ([black head, hair]), as synthesize.py runs them.  Reports kernel-only and
end-to-end ms per view of the pair, the dropped count, the host normal estimate of the 10^6 hair vertices, and the CPU path's
seconds per view at a reduced size.  One JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(n_strands, n_verts, W, H, views):
    import synthetic
    from synthesize import camera_matrices, lighting
    from scene.mesh_renderer import MeshModel
    from tests.synth_fixtures import sphere_mesh
    from utils.camera import generate_cameras
    walks = synthetic.strand_polylines(n_strands, n_verts - 1, seed=0)
    verts = walks.reshape(-1, 3).astype(np.float64)
    base = np.arange(n_strands)[:, None] * n_verts + np.arange(n_verts - 1)[None]
    edges = np.stack([base, base + 1], -1).reshape(-1, 2)
    cols = np.repeat(np.array([[0.545, 0.271, 0.075, 1], [0.639, 0.341, 0.125, 1], [0.561, 0.388, 0.196, 1]])[np.arange(n_strands) % 3],
                     n_verts, 0)
    v, f, n = sphere_mesh(0.095, 100, 100)
    t0 = time.time()
    from utils.normals import estimate_pointcloud_normals
    nrm = estimate_pointcloud_normals(verts)
    t_norm = time.time() - t0
    models = [MeshModel(v, faces=f, colors=np.zeros(4), normals=n, use_lighting=False),
              MeshModel(v, faces=f, colors=np.array([0.75, 0.75, 0.75, 1]), normals=n),
              MeshModel(verts, edges=edges, colors=cols, normals=nrm)]
    cy = (verts[:, 1].max() + verts[:, 1].min()) / 2
    pose = np.eye(4)
    pose[:3, 3] = [0, cy, 0.5]
    pose[:3, 1:3] *= -1
    cams, Es = generate_cameras(views, H, W, cam_pose=pose, anchor_pos=np.array([0, cy, 0]), offset=0.5)
    _, vw, pj = camera_matrices(cams, Es)
    return models, lighting(), vw, pj, t_norm, edges.shape[0], f.shape[0]


def main():
    import torch
    import hgs_runtime as rt
    from scene._raster_device import DeviceMeshes
    from scene.mesh_renderer import _Prepared, render_views
    W = H = 1000
    V = 16
    models, light, vw, pj, t_norm, n_seg, n_tri = scene(10000, 100, W, H, V)
    states = {k: DeviceMeshes(_Prepared(models, list(k)), "cuda") for k in ((1, 2), (0, 2))}

    def pair():
        a = render_views(models, vw, pj, W, H, light, mesh_indices=[1, 2], device="cuda", return_gray=True, _device_state=states[(1, 2)])
        b = render_views(models, vw, pj, W, H, light, mesh_indices=[0, 2], device="cuda", _device_state=states[(0, 2)])
        return a[1] + b[1], a[0]

    dropped, img = pair()
    torch.cuda.synchronize()
    e2e = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pair()
        torch.cuda.synchronize()
        e2e.append((time.perf_counter() - t0) * 1e3 / V)
    # kernel-only: the four launches of each render, timed with events around the same calls
    from scene import _raster_device as D
    kern = []
    for _ in range(5):
        t = 0.0
        for k in ((1, 2), (0, 2)):
            dm = states[k]
            L = rt.lib()
            T = int(L.hgs_raster_tiles(W, H))
            vwt = torch.from_numpy(np.ascontiguousarray(vw.astype(np.float32).astype(np.float64).reshape(V, 16))).cuda()
            pjt = torch.from_numpy(np.ascontiguousarray(pj.astype(np.float32).astype(np.float64).reshape(V, 16))).cuda()
            vout = torch.empty(V * dm.NV * int(L.hgs_raster_vertex_bytes()), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(V * T, dtype=torch.int32, device="cuda")
            drop = torch.zeros(1, dtype=torch.int64, device="cuda")
            s = rt.current_stream()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            rt.check(L.hgs_raster_vertices(s, V, dm.NV, W, H, rt.ptr(dm.pw), rt.ptr(vwt), rt.ptr(pjt), rt.ptr(vout)))
            rt.check(L.hgs_raster_count(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), dm.NV, rt.ptr(vout),
                                        rt.ptr(counts), rt.ptr(drop)))
            ev[1].record()
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            offs = ends - counts
            total = int(ends[-1])
            lst = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            cur = torch.zeros(V * T, dtype=torch.int32, device="cuda")
            rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device="cuda")
            gray = torch.empty((V, H, W), dtype=torch.uint8, device="cuda")
            import ctypes as C
            lh = (C.c_double * 9)(*light.packed())
            bh = (C.c_ubyte * 3)(0, 0, 0)
            ev[2].record()
            rt.check(L.hgs_raster_fill(s, V, W, H, dm.n_models, rt.ptr(dm.models), dm.n_prims, rt.ptr(dm.idx), dm.NV, rt.ptr(vout),
                                       rt.ptr(counts), rt.ptr(offs), rt.ptr(cur), rt.ptr(lst)))
            rt.check(L.hgs_raster_resolve(s, V, W, H, dm.n_models, rt.ptr(dm.models), rt.ptr(dm.idx), dm.NV, rt.ptr(vout), rt.ptr(dm.pw),
                                          rt.ptr(dm.nw), rt.ptr(dm.col), lh, bh, rt.ptr(counts), rt.ptr(offs), rt.ptr(lst), rt.ptr(rgb),
                                          rt.ptr(gray) if k == (1, 2) else None))
            ev[3].record()
            torch.cuda.synchronize()
            t += ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3])
            if k == (1, 2):
                entries = total
        kern.append(t / V)
    # CPU path at a reduced size: 2000 strands, 250x250, 2 views
    cm, cl, cvw, cpj, _, _, _ = scene(2000, 100, 250, 250, 2)
    t0 = time.time()
    render_views(cm, cvw, cpj, 250, 250, cl, mesh_indices=[1, 2])
    render_views(cm, cvw, cpj, 250, 250, cl, mesh_indices=[0, 2])
    cpu = (time.time() - t0) / 2
    print(json.dumps({"views": V, "size": [W, H], "segments": n_seg, "triangles": n_tri, "dropped": dropped,
                      "tile_list_entries_image": entries, "hair_pixels_view0": int((img[0] != 0).any(-1).sum()),
                      "kernel_ms_per_view_pair": round(float(np.median(kern)), 3), "e2e_ms_per_view_pair": round(float(np.median(e2e)), 3),
                      "host_normals_s_1e6": round(t_norm, 2), "cpu_s_per_view_pair_250px_2000strands": round(cpu, 2)}))


if __name__ == "__main__":
    main()
