"""Time of the undistortion (csrc/hgs_undistort.hip through utils/undistort.py) for one batch of --views images of 1920x1080, 3
channels, seen through an OPENCV camera: GPU ms per batch kernel-only (hgs_undistort_images between device events, inputs and outputs
resident), end to end (host uint8 [N, H, W, 3] -> host images and validity plane, copies included) and the numpy path's seconds per
batch on the same box.  Each figure is the median of its repeats after one warm-up.  Input: seeded noise.  Prints one JSON line and
writes it to profiles/undistort_timing.json (--out).
  python tools/undistort_timing.py [--views 48] [--reps 9] [--cpu_reps 3] [--out profiles/undistort_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np

W, H, C = 1920, 1080, 3


def cameras():
    from data.colmap import Camera
    from utils.undistort import undistorted_camera
    cam = Camera(1, "OPENCV", W, H, np.array([1500.0, 1510.0, 975.0, 530.0, -0.18, 0.06, 0.004, -0.003]))
    return cam, undistorted_camera(cam)


def kernel_only(images, cam, out_cam, reps):
    """ms per call on resident buffers, between device events."""
    import torch
    from utils.undistort import undistort_device
    src = torch.from_numpy(images).cuda()
    undistort_device(src, cam, out_cam, "bilinear")
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        undistort_device(src, cam, out_cam, "bilinear")
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def end_to_end(images, cam, out_cam, reps, device):
    """ms per call of undistort_images, host arrays in and out."""
    from utils.undistort import undistort_images
    if device is not None:
        import torch
        undistort_images(images, cam, out_cam, "bilinear", device=device)
    ts = []
    for _ in range(reps):
        if device is not None:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        undistort_images(images, cam, out_cam, "bilinear", device=device)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=48)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "undistort_timing.py measures the GPU path: it needs the GPU"
    cam, out_cam = cameras()
    images = np.random.default_rng(0).integers(0, 256, (a.views, H, W, C), dtype=np.uint8)
    traffic = a.views * C * (W * H + out_cam.width * out_cam.height)
    k_ms = kernel_only(images, cam, out_cam, a.reps)
    res = {"views": a.views, "reps": a.reps, "source": [W, H, C], "model": cam.model, "output": [out_cam.width, out_cam.height],
           "device": torch.cuda.get_device_name(0), "bytes_read_once_and_written_once": traffic,
           "kernel_ms_per_batch": round(k_ms, 3), "kernel_GB_per_s": round(traffic / k_ms / 1e6, 1),
           "e2e_ms_per_batch": round(end_to_end(images, cam, out_cam, a.reps, "cuda"), 2)}
    if a.cpu_reps > 0:
        res["numpy_s_per_batch"] = round(end_to_end(images, cam, out_cam, a.cpu_reps, None) / 1e3, 2)
        res["cpu_reps"] = a.cpu_reps
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
