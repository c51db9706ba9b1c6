#!/usr/bin/env python3
"""Times one deduplication of exported strands (scene/strand_dedupe.py, csrc/hgs_dedupe.hip): --strands strands (10^5) of --points points
(100), random walks of 2 mm steps rooted on the upper half of a sphere of 10 cm (a scalp: the roots lie on a surface, so the root test
passes far more often than in a volume), of which --copies (0.2) are copies of an earlier strand with every coordinate jittered by at
most --jitter (0.1 mm), at --dist 0.3 mm; everything from seed 0.  After a warm-up of each path, in this one process: the count and the
fill pass on their own (device events around --repeats back-to-back launches on resident buffers, the time per launch;
five such windows; median and spread reported), every resolve round on its own (device events around the one launch), the device path
end to end (dedupe_strands(device="cuda"): uploads, count, cumsum, fill, the rounds with their reads, the copies to the host, the
selection and the report; wall clock around a synchronised call, five calls), the numpy path on the first --host-strands (10^4) strands
(wall clock) with a check that the device path yields the same bytes there, and, for honesty, the ROOT test alone as a plain torch
statement on the same device: torch.cdist of the roots in float64, --chunk rows at a time against all earlier roots, thresholded and
counted -- what the search would cost without a kernel of its own, before any other joint is looked at (its distances are not the
contract's bits).  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(N, M, copies, jitter, seed=0):
    """A StrandExport of N strands of M points: random walks from a half sphere, a share `copies` of them jittered copies of earlier ones."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(N, 3))
    d[:, 2] = np.abs(d[:, 2])
    steps = 2e-3 * rng.normal(size=(N, M, 3))
    steps[:, 0] = 0.1 * d / np.linalg.norm(d, axis=1, keepdims=True)
    x = np.cumsum(steps, axis=1)
    is_copy = rng.uniform(size=N) < copies
    is_copy[0] = False
    src = (rng.uniform(size=N) * np.arange(N)).astype(np.int64)
    for i in np.nonzero(is_copy)[0]:                                                # in ascending order: a copy of a copy is a copy
        x[i] = x[src[i]] + rng.uniform(-jitter, jitter, (M, 3))
    pts = x.reshape(-1, 3).astype(np.float32)
    attrs = rng.uniform(0.0, 1.0, (pts.shape[0], 5)).astype(np.float32)
    return StrandExport(pts, attrs, np.arange(N + 1, dtype=np.int64) * M, np.arange(N, dtype=np.int64), np.zeros(N)), int(is_copy.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--copies", type=float, default=0.2)
    ap.add_argument("--jitter", type=float, default=1e-4)
    ap.add_argument("--dist", type=float, default=3e-4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-strands", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import strand_dedupe as SD
    from scene.strand_simplify import take_strands
    strands, n_copies = scene(args.strands, args.points, args.copies, args.jitter)
    N, M, tol = args.strands, args.points, args.dist
    p = torch.as_tensor(strands.points, device="cuda")

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    def window(fn):
        def run():
            for _ in range(args.repeats):
                fn()
        return events(run)[0] / args.repeats

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    counts = SD.count_device(p, N, M, tol)                                          # warm-up, and the buffers the windows run on
    ends = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
    starts, n_pairs = (ends - counts.view(-1)).contiguous(), int(ends[-1])
    SD.fill_device(p, N, M, tol, starts, n_pairs)
    times = {"count": [], "fill": []}
    for _ in range(5):
        times["count"].append(window(lambda: SD.count_device(p, N, M, tol)))
        times["fill"].append(window(lambda: SD.fill_device(p, N, M, tol, starts, n_pairs)))
    # the resolve rounds, one launch each
    lower_offsets, lower = SD.pairs_device(p, N, M, tol)
    state = (lower_offsets[1:] == lower_offsets[:-1]).to(torch.uint8)
    other = torch.empty_like(state)
    kept_by, rounds = torch.arange(N, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    round_ms, left = [], []
    while lower.shape[0] and (not left or left[-1]):
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        r = len(round_ms) + 1
        round_ms.append(round(events(lambda: SD.resolve_round_device(lower_offsets, lower, state, other, r, kept_by, rounds, word))[0], 4))
        left.append(int(word))
        state, other = other, state

    def e2e_s(s, device):
        if device is not None:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SD.dedupe_strands(s, tol, device=device)
        return time.perf_counter() - t0, res

    e2e_s(strands, "cuda")
    e2e = []
    for _ in range(5):
        t, (res, report) = e2e_s(strands, "cuda")
        e2e.append(t)
    # the root test alone as a torch statement
    roots = p.view(N, M, 3)[:, 0].to(torch.float64).contiguous()

    def cdist_roots():
        total = torch.zeros((), dtype=torch.int64, device="cuda")
        for a in range(0, N, args.chunk):
            b = min(N, a + args.chunk)
            hit = torch.cdist(roots[a:b], roots[:b]) <= tol
            total += torch.tril(hit, diagonal=a - 1).sum()
        return int(total)

    cdist_roots()
    cdist = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        close = cdist_roots()
        cdist.append((time.perf_counter() - t0) * 1e3)
    result = {"strands": N, "points_per_strand": M, "copies": n_copies, "jitter": args.jitter, "dist": tol, "gpu": torch.cuda.get_device_name(0),
              "root_tests": N * (N - 1) // 2, "pairs": int(lower.shape[0]), "report": report,
              "count_ms": stats(times["count"]), "fill_ms": stats(times["fill"]),
              "resolve_round_ms": round_ms, "undecided_after_round": left, "device_e2e_s": stats(e2e),
              "torch_cdist_root_test_ms": stats(cdist), "torch_cdist_close_roots": close}
    if not args.device_only:
        few = take_strands(strands, np.arange(min(N, args.host_strands)))
        t, (hres, hreport) = e2e_s(few, None)
        _, (dres, dreport) = e2e_s(few, "cuda")
        result["numpy_s_first_strands"] = {"strands": few.n_strands, "seconds": round(t, 3), "report": hreport}
        result["paths_agree_bytewise"] = bool(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(dres, hres)) and dreport == hreport)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
