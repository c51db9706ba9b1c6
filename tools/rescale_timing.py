"""Time of the rescaling (csrc/hgs_rescale.hip through utils/rescale.py) for --views views of 3208 x 2200 -- the RGB image, the mask and
the orientation / confidence pair of each -- brought to half size: GPU ms per kernel alone (hgs_rescale_images on the images, on the
masks, hgs_rescale_orientation on the pairs gated by the masks; between device events, inputs and outputs resident, with the bytes
each reads once and writes once per second), the device path end to end (host arrays in, host arrays out, copies included), the numpy
path's seconds on the same arrays and, for context only, PIL's resize of the same RGB images (its default filter, as the loader calls
it).  Each GPU figure is the median of its repeats after one warm-up.  Input: seeded noise images, blocky masks, coherent orientation
planes.  Prints one JSON line and writes it to profiles/rescale_timing.json (--out).
  python tools/rescale_timing.py [--views 64] [--reps 9] [--cpu_reps 1] [--out profiles/rescale_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np

W, H = 3208, 2200
WD, HD = W // 2, H // 2


def planes(views):
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (views, H, W, 3), dtype=np.uint8)
    small = rng.integers(0, 2, (views, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8) * 255
    masks = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)[:, :H, :W])
    y, x = np.mgrid[0:H, 0:W]
    ramp = ((x + 2 * y) // 3).astype(np.int16)
    angle = np.stack([(ramp + rng.integers(0, 256) + rng.integers(-2, 3, (H, W), dtype=np.int16)).astype(np.uint8) for _ in range(views)])
    conf = rng.integers(0, 256, (views, H, W), dtype=np.uint8)
    return images, masks, angle, conf


def device_ms(fn, reps):
    """Median ms of fn() between device events, after one warm-up."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def host_ms(fn, reps, sync=False):
    """Median ms of fn() by the host clock (after one warm-up where the device is involved)."""
    if sync:
        import torch
        fn()
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu_reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescale_timing.json"))
    a = ap.parse_args()
    import torch
    from PIL import Image
    from utils.rescale import orientation_tables, rescale_device, rescale_images, rescale_orientation, rescale_orientation_device
    assert torch.cuda.is_available(), "rescale_timing.py measures the GPU path: it needs the GPU"
    images, masks, angle, conf = planes(a.views)
    size = (WD, HD)
    d_images, d_masks = torch.from_numpy(images).cuda(), torch.from_numpy(masks).cuda()
    d_angle, d_conf = torch.from_numpy(angle).cuda(), torch.from_numpy(conf).cuda()
    tables = torch.from_numpy(orientation_tables()).cuda()
    px, pxd = a.views * W * H, a.views * WD * HD
    kernels = {"images_rgb_average": (lambda: rescale_device(d_images, size, "average"), 3 * (px + pxd)),
               "masks_threshold": (lambda: rescale_device(d_masks[..., None], size, "threshold"), px + pxd),
               "orientation_pairs_masked": (lambda: rescale_orientation_device(d_angle, d_conf, d_masks, size, tables), 3 * px + 2 * pxd)}
    res = {"views": a.views, "reps": a.reps, "source": [W, H], "output": [WD, HD], "device": torch.cuda.get_device_name(0)}
    for name, (fn, traffic) in kernels.items():
        ms = device_ms(fn, a.reps)
        res[name] = {"bytes_read_once_and_written_once": traffic, "kernel_ms": round(ms, 3), "GB_per_s": round(traffic / ms / 1e6, 1)}
    del d_images, d_masks, d_angle, d_conf

    def everything(device):
        rescale_images(images, size, "average", device=device)
        rescale_images(masks[..., None], size, "threshold", device=device)
        rescale_orientation(angle, conf, masks, size, device=device)
    res["e2e_ms"] = round(host_ms(lambda: everything("cuda"), a.reps, sync=True), 1)
    if a.cpu_reps > 0:
        res["numpy_s"] = round(host_ms(lambda: everything(None), a.cpu_reps) / 1e3, 1)
        res["pil_resize_rgb_s"] = round(host_ms(lambda: [Image.fromarray(im).resize(size) for im in images], a.cpu_reps) / 1e3, 2)
        res["cpu_reps"] = a.cpu_reps
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
