"""Time of the image metrics (csrc/hgs_view_stats.hip through loss/image_metrics.py, and the view_metrics.py driver) for 48 views at
1920x1080 and 16 at 1000x1000:
  * kernel: hgs_view_stats alone on resident seeded planes (every plane present: 49 bytes read per pixel -- pred and gt 12 each,
    mask 1, fg 4, omap 12, gt angle 4, confidence 4), one launch per --batch views, between device events after one warm-up; the
    median of --reps, per view, and the bytes per second it implies (against the 8 TB/s of HBM);
  * driver: score_cameras (render_multi + the kernel + the fused SSIM per view, results on the host) over a capture of that many
    views written by the tests' _write_capture (random images, masks and orientation maps) and its input cloud, per view; and
    view_metrics.main end to end (Scene loading included), per view.
Prints one JSON line.
  python tools/view_metrics_timing.py [--reps 10] [--batch 8]"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

BYTES_PER_PIXEL = 3 * 4 + 3 * 4 + 1 + 4 + 3 * 4 + 4 + 4


def kernel_only(V, H, W, batch, reps):
    import torch
    import hgs_runtime as rt
    from loss.image_metrics import STATS
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)   # noqa: E731
    pred, gt, fg, omap = r(V, 3, H, W), r(V, 3, H, W), r(V, H, W), r(V, 3, H, W) * 2 - 1
    mask = (r(V, H, W) > 0.5).to(torch.uint8)
    theta, conf = r(V, H, W) * 3.14159, r(V, H, W)
    vm = torch.eye(4, device=dev).repeat(V, 1, 1).reshape(V, 16).contiguous()
    L = rt.lib()
    nb = L.hgs_view_stats_num_blocks(H, W)
    partials = torch.empty((V, nb, len(STATS)), dtype=torch.float64, device=dev)
    out = torch.empty((V, len(STATS)), dtype=torch.float64, device=dev)

    def call():
        s = rt.current_stream()
        for b0 in range(0, V, batch):
            n = min(batch, V - b0)
            rt.check(L.hgs_view_stats(s, n, H, W, rt.ptr(pred[b0:]), rt.ptr(gt[b0:]), rt.ptr(mask[b0:]), rt.ptr(fg[b0:]), 0.5,
                                      rt.ptr(omap[b0:]), rt.ptr(vm[b0:]), rt.ptr(theta[b0:]), rt.ptr(conf[b0:]), 1e-7,
                                      rt.ptr(partials[b0:]), rt.ptr(out[b0:])))
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
    ms = statistics.median(ts)
    tbs = V * H * W * BYTES_PER_PIXEL / (ms * 1e-3) / 1e12
    return {"kernel_ms_per_view": round(ms / V, 4), "kernel_TBps": round(tbs, 2), "share_of_8TBps": round(tbs / 8.0, 3)}


def driver(V, H, W, batch, reps):
    import torch
    import view_metrics as cli
    from loss.image_metrics import score_cameras
    from scene import Scene
    from tests.test_dataset_io_cpu import _write_capture
    with tempfile.TemporaryDirectory() as tmp:
        src, model = pathlib.Path(tmp) / "capture", pathlib.Path(tmp) / "model"
        _write_capture(src, n_views=V, W=W, H=H)
        args = cli.parse_args(["-s", str(src), "-m", str(model), "-r", "1", "--quiet"])   # (-r 1: true 1080p)
        scene = Scene(args, shuffle=False)
        scene.save(0)                                # (the input cloud as iteration_0: what the driver loads)
        cams = scene.getCameras()
        score_cameras(cams, scene.gaussians, batch=batch)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score_cameras(cams, scene.gaussians, batch=batch)
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        cli.main(["-s", str(src), "-m", str(model), "-r", "1", "--batch", str(batch), "--quiet"])
        e2e = time.perf_counter() - t0
    return {"score_ms_per_view": round(statistics.median(ts) * 1e3 / V, 3), "main_ms_per_view": round(e2e * 1e3 / V, 2),
            "points": int(scene.gaussians.get_xyz.shape[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "view_metrics_timing.py measures the GPU path: it needs the GPU"
    res = {"reps": a.reps, "batch": a.batch, "bytes_per_pixel": BYTES_PER_PIXEL}
    for V, W, H in ((48, 1920, 1080), (16, 1000, 1000)):
        row = {"views": V}
        row.update(kernel_only(V, H, W, a.batch, a.reps))
        row.update(driver(V, H, W, a.batch, max(1, a.reps // 2)))
        res[f"{W}x{H}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
