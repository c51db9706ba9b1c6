"""Time of the orientation maps (csrc/hgs_vision.hip through utils/vision.py) for 16-view batches at 1000x1000 and 1920x1080:
GPU ms per view kernel-only (hgs_orientation_field + hgs_orientation_confidence between device events, inputs resident) and end to
end (host uint8 [N, H, W] -> host field and confidence arrays), plus the CPU path's seconds per view at 1000x1000.  Each figure is
the median of --reps after one warm-up.  Input: gray uint8 of RGB renders of a synthetic.build_capture strand model (--input
render), or seeded noise (--input noise).  Prints one JSON line.
  python tools/orientation_timing.py [--views 16] [--reps 5] [--input render|noise] [--cpu_reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np


def views(kind, n, W, H):
    import torch
    from utils.vision import to_gray
    if kind == "noise":
        return np.random.default_rng(0).integers(0, 256, (n, H, W), dtype=np.uint8)
    from synthetic import build_capture
    _, _, cams, _ = build_capture((1000, False, n, W, H), seed=0)
    return np.stack([to_gray((c.original_image.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy())
                     for c in cams])


def kernel_only(gray_host, reps):
    """ms per call of the two entry points on resident buffers, between device events."""
    import torch
    import hgs_runtime as rt
    from utils.vision import gabor_kernels
    N, H, W = gray_host.shape
    thetas, kernels = gabor_kernels()
    A, side = kernels.shape[0], kernels.shape[1]
    dev = torch.device("cuda")
    gray = torch.from_numpy(gray_host).to(dev)
    th = torch.from_numpy(thetas).to(dev)
    w = torch.from_numpy(kernels.astype(np.float64)).to(dev)
    idx = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    var = torch.empty((N, H, W), dtype=torch.float64, device=dev)
    conf = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    maxinv = torch.empty(N, dtype=torch.float64, device=dev)
    L = rt.lib()
    scratch = torch.empty(int(L.hgs_orientation_scratch_bytes(N, H, W, A, side)), dtype=torch.uint8, device=dev)

    def call():
        s = rt.current_stream()
        rt.check(L.hgs_orientation_field(s, N, H, W, rt.ptr(gray), A, side, rt.ptr(w), rt.ptr(th), rt.ptr(idx), rt.ptr(var),
                                         rt.ptr(maxinv), None, rt.ptr(scratch), scratch.numel()))
        rt.check(L.hgs_orientation_confidence(s, N, H, W, rt.ptr(var), rt.ptr(maxinv), rt.ptr(conf)))
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def end_to_end(gray_host, reps):
    import torch
    from utils.vision import estimate_orientation_fields

    def call():
        f, c = estimate_orientation_fields(torch.from_numpy(gray_host).cuda())
        return f.cpu().numpy(), c.cpu().numpy()
    call()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu_reps", type=int, default=5)
    ap.add_argument("--input", default="render", choices=["render", "noise"])
    a = ap.parse_args()
    import torch
    from utils.vision import estimate_orientation_field
    assert torch.cuda.is_available(), "orientation_timing.py measures the GPU path: it needs the GPU"
    res = {"views": a.views, "reps": a.reps, "input": a.input}
    for W, H in ((1000, 1000), (1920, 1080)):
        g = views(a.input, a.views, W, H)
        k_ms = kernel_only(g, a.reps)
        e_ms = end_to_end(g, a.reps)
        res[f"{W}x{H}"] = {"kernel_ms_per_view": round(k_ms / a.views, 3), "e2e_ms_per_view": round(e_ms / a.views, 3),
                           "fma_per_view": int(H * W * 180 * 31 * 31)}
        if W == 1000 and a.cpu_reps > 0:
            estimate_orientation_field(np.random.default_rng(0).integers(0, 256, (64, 64), dtype=np.uint8))   # (scipy's imports)
            ts = []
            for _ in range(a.cpu_reps):
                t0 = time.perf_counter()
                estimate_orientation_field(g[0])
                ts.append(time.perf_counter() - t0)
            res[f"{W}x{H}"]["cpu_s_per_view"] = round(statistics.median(ts), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
