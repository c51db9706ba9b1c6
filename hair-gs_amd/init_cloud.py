#!/usr/bin/env python3
"""Carves the point cloud Stage I starts from out of a capture's hair masks (utils/carve.py states the arithmetic): COLMAP's own
cloud is sparse where hair is and dense on the face, the shoulders and the background.
  python init_cloud.py -s <scene> [--mode hull|filter|both] [--grid 256] [--bounds x0 y0 z0 x1 y1 z1]
                       [--min_views 3] [--min_percent 50] [--dilate 0] [--no_shell] [--max_points 200000]
                       [--images images] [--device cuda|cpu] [--overwrite]
                       [--directions [--orientations orientations] [--rounds 3] [--sigma_deg 10] [--min_conf 1] [--min_coherence 0]
                                     [--visibility [--vis_skip 1] [--vis_max_blocked 0]]]
Reads <scene>/sparse/0 (binary or text; PINHOLE and SIMPLE_PINHOLE cameras only -- undistort.py makes them), <scene>/masks/<name> for
every image of the model and, for the hull's colours, <scene>/<images>/<name> (data/capture.py forms the names, as for the loader).
  hull    a --grid voxel grid over the automatic bounds (utils.carve.auto_bounds) or over --bounds is tested against every mask; a voxel
          is kept where at least --min_views views have its centre in frame and --min_percent percent of those see hair there; of the
          kept voxels the shell (a face neighbour empty or outside) is written unless --no_shell.  More than --max_points voxels: those
          at flat indices floor(j*n/max_points), j = 0..max_points - 1, of the ascending voxel order.  Points are the float64 voxel
          centres, colours the rounded mean (sum + hits//2)//hits of the image pixels under the hits (128 without a hit), error 0.
  filter  the scene's COLMAP points, voted with the same rule; the kept ones keep their colours and errors.
  both    the filtered points followed by the hull's.
--min_percent 50 suits a 360-degree capture, where the head hides the far side's hair from half the ring; it is a knob, and 100 is the
classical visual hull.  --dilate r widens every mask by r pixels first (1-pixel strands leave holes in a mask).
The write is in place and loses nothing: on the first run sparse/0/points3D.bin (or .txt) is renamed to points3D.colmap.bin (.txt) --
a scene without points gets an empty points3D.colmap.bin -- and later runs read the COLMAP points from that backup and refuse to
replace their predecessor's result without --overwrite.  The new points3D.bin is written under a temporary name and renamed into
place; the loader's points3D.ply conversion of the old points is removed.  The points get ids 1..n and empty tracks: the point ids
that images.bin refers to become stale, and nothing in this project reads them.  main() returns the number of points written.
--directions also lifts a 3-D hair direction for every written point from the views' orientation maps (utils/lift.py states the
arithmetic): <scene>/<orientations>/<stem>_orientation.png and _confidence.png of every view are read (orient.py writes them), the
views that have the point in frame, on the (dilated) mask and with a confidence of at least --min_conf vote in --rounds re-weighted
rounds of scale --sigma_deg, and sparse/0/points3D.ply is written with the same points and colours and the direction in nx, ny, nz --
zero where fewer than two views determine it or its coherence is below --min_coherence.  The loader reads that file as it is, and
training with --init_directions starts from Gaussians stretched along it.  Without the flag no points3D.ply is written.
--visibility (with --directions, modes hull and both) lets a view vote for a point's direction only where it can see the point: a ray
from the point to the camera is marched through the solid carved grid (utils/visibility.py states the arithmetic), and a view whose
ray meets more than --vis_max_blocked occupied voxels further than --vis_skip voxels from the point's own is left out.  A filtered
COLMAP point outside the grid is unoccluded.  A point left with fewer than two views gets the zero direction; the counts are printed.
Without the flag every file is written as before."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

BACKUPS = ("points3D.colmap.bin", "points3D.colmap.txt")


def mean_colours(rgb_sum, hits):
    """(sum + hits//2)//hits per channel, 128 where hits == 0; uint8 [n, 3]."""
    hits = np.asarray(hits, np.int64)
    safe = np.maximum(hits, 1)[:, None]
    rgb = (np.asarray(rgb_sum, np.int64) + (hits // 2)[:, None]) // safe
    return np.where((hits > 0)[:, None], rgb, 128).astype(np.uint8)


def _fail(msg):
    raise SystemExit(f"init_cloud.py: {msg}")


def lift_normals(voter, orients, confs, xyz, args, grid=None):
    """(normals f64 [n, 3], coherence f64 [n]) of the written points: utils.lift's directions, zero below --min_coherence.  grid
    (origin, h, dims, occ), the solid carved grid: the votes are gated by utils.visibility's march through it, and what the gate did is
    printed."""
    from utils import lift, visibility
    knobs = (args.rounds, args.sigma_deg, args.min_conf)
    visible = plain = None
    if voter.device is None:
        if grid is not None:
            origin, h, _, occ = grid
            visible = visibility.visibility_numpy(xyz, visibility.camera_centres(voter.views), occ, origin, h, args.vis_skip, args.vis_max_blocked)
            plain = lift.moments_numpy(xyz, voter.views, voter.masks, orients, confs, min_conf=args.min_conf)[2]
        d, coherence, count = lift.lift_directions(xyz, voter.views, voter.masks, orients, confs, *knobs, visible=visible)
    else:
        import torch
        from utils.views import upload_points
        packed = lift.pack(voter.views, voter.masks, orients, confs, voter.device, carve_packed=voter.packed)
        pts = upload_points(xyz, voter.device)
        words = None
        if grid is not None:
            origin, h, _, occ = grid
            centres = visibility.upload_centres(visibility.camera_centres(voter.views), voter.device)
            words = visibility.visibility_device(pts, centres, torch.from_numpy(occ).to(voter.device), origin, h, args.vis_skip,
                                                 args.vis_max_blocked)
            visible = words.cpu().numpy()
            plain = lift.moments_device(pts, packed, min_conf=args.min_conf)[2].cpu().numpy()
        d, coherence, count = (t.cpu().numpy() for t in lift.directions_device(pts, packed, *knobs, visible=words))
    if grid is not None:                                         # (plain: the views the lift would use without the gate)
        on_mask, seen = visibility.pair_counts(xyz, voter.views, voter.masks, visible)
        print(f"visibility (skip {args.vis_skip}, max_blocked {args.vis_max_blocked}): {on_mask} (point, view) pair(s) in frame and on the mask, "
              f"{seen} of them visible; {int(((plain >= 2) & (count < 2)).sum())} point(s) lost their direction to the gate")
    return np.where((coherence >= args.min_coherence)[:, None], d, 0.0), coherence


class _Voter:
    """The capture's views behind one device convention: numpy arrays, or buffers packed once on the GPU."""

    def __init__(self, views, masks, images, device, dilate_r):
        from utils import carve
        self.carve, self.views, self.device = carve, views, device
        if device is None:
            self.masks = [carve.dilate_numpy(m, dilate_r) for m in masks] if dilate_r else masks
            self.images = images
        else:
            import torch
            if dilate_r:
                masks = [carve.dilate_device(torch.from_numpy(m).to(device), dilate_r).cpu().numpy() for m in masks]
            self.masks, self.images = masks, images
            self.packed = carve.pack(views, masks, images, device)

    def grid(self, origin, h, dims, min_views, min_percent):
        if self.device is None:
            return self.carve.grid_numpy(origin, h, dims, self.views, self.masks, min_views, min_percent)
        return self.carve.grid_device(origin, h, dims, self.packed, min_views, min_percent).cpu().numpy()

    def shell(self, occ):
        if self.device is None:
            return self.carve.shell_numpy(occ)
        import torch
        return self.carve.shell_device(torch.from_numpy(occ).to(self.device)).cpu().numpy()

    def votes(self, points, with_rgb):
        if self.device is None:
            return self.carve.votes_numpy(points, self.views, self.masks, self.images if with_rgb else None)
        pts = self.carve.upload_points(points, self.device)
        return tuple(t.cpu().numpy() for t in self.carve.votes_device(pts, self.packed, with_rgb=with_rgb))


def hull_grid(voter, bounds, grid, min_views, min_percent):
    """(lo, hi, how, origin, h, dims, occ) of the carved grid over the given or the automatic bounds; occ is a host array."""
    carve = voter.carve
    if bounds is not None:
        lo, hi, how = np.array(bounds[:3], np.float64), np.array(bounds[3:], np.float64), "given"
    else:
        try:
            lo, hi = carve.auto_bounds(voter.views, voter.masks, min_views, min_percent,
                                       carve=lambda o, h, d: voter.grid(o, h, d, min_views, min_percent))
        except ValueError as e:
            _fail(f"{e} (min_views = {min_views}, min_percent = {min_percent}; --dilate widens thin masks, --bounds skips the search)")
        how = "automatic"
    try:
        origin, h, dims = carve.fine_grid(lo, hi, grid)
        occ = voter.grid(origin, h, dims, min_views, min_percent)
    except ValueError as e:
        _fail(str(e))
    return lo, hi, how, origin, h, dims, occ


def hull_points(voter, args):
    """(xyz f64 [n, 3], rgb u8 [n, 3], (origin, h, dims, occ)) of the carved grid, occ the solid one; prints what it did."""
    lo, hi, how, origin, h, dims, occ = hull_grid(voter, args.bounds, args.grid, args.min_views, args.min_percent)
    kept = int(np.count_nonzero(occ))
    out = occ if args.no_shell else voter.shell(occ)
    flat = np.flatnonzero(out)
    n_shell = flat.size
    flat = flat[voter.carve.select(flat.size, args.max_points)]
    nx, ny, nz = dims
    xs, ys, zs = voter.carve.centres(origin, h, dims)
    xyz = np.stack([xs[flat % nx], ys[(flat // nx) % ny], zs[flat // (nx * ny)]], axis=1)
    _, hits, rgb_sum = voter.votes(xyz, True) if flat.size else (None, np.zeros(0, np.int32), np.zeros((0, 3), np.int32))
    print(f"bounds ({how}): {lo.tolist()} .. {hi.tolist()}")
    print(f"grid {nx} x {ny} x {nz}, voxel size {h:.6g}: {kept} kept, {n_shell} {'kept (no shell)' if args.no_shell else 'on the shell'}, "
          f"{flat.size} written")
    return xyz, mean_colours(rgb_sum, hits), (origin, h, dims, occ)


def main(argv=None):
    from data import capture
    parser = ArgumentParser(description="Carve the Stage-I point cloud from a capture's hair masks")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (sparse/0, masks/, <images>/)")
    parser.add_argument("--mode", default="hull", choices=("hull", "filter", "both"))
    parser.add_argument("--grid", type=int, default=256, help="voxels along the longest side of the bounds")
    parser.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("x0", "y0", "z0", "x1", "y1", "z1"))
    parser.add_argument("--min_views", type=int, default=3)
    parser.add_argument("--min_percent", type=int, default=50)
    parser.add_argument("--dilate", type=int, default=0, help="widen every mask by this many pixels first")
    parser.add_argument("--no_shell", action="store_true", help="write every kept voxel, not only the shell")
    parser.add_argument("--max_points", type=int, default=200000)
    parser.add_argument("--images", "-i", default="images")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--overwrite", action="store_true")
    parser.add_argument("--directions", action="store_true", help="also lift hair directions into sparse/0/points3D.ply's normals")
    parser.add_argument("--orientations", default="orientations", help=f"folder of the <stem>{capture.ORIENTATION} / {capture.CONFIDENCE} maps")
    parser.add_argument("--rounds", type=int, default=3, help="re-weighted rounds after the plain least-squares one")
    parser.add_argument("--sigma_deg", type=float, default=10.0, help="angular scale of the re-weighting")
    parser.add_argument("--min_conf", type=int, default=1, help="smallest confidence byte (0 to 255) that votes")
    parser.add_argument("--min_coherence", type=float, default=0.0, help="directions below this coherence are written as zero")
    parser.add_argument("--visibility", action="store_true", help="with --directions: only views that see a point through the carved hull vote")
    parser.add_argument("--vis_skip", type=int, default=1, help="occupied voxels within this many voxels of the point's own do not block")
    parser.add_argument("--vis_max_blocked", type=int, default=0, help="occupied voxels a ray may meet before its view is left out")
    args = parser.parse_args(argv)
    from data.colmap import read_points3D_binary, read_points3D_text, write_points3D_arrays
    from utils import carve
    from utils.views import load_views, read_plane
    if args.device not in ("cuda", "cpu"):
        _fail(f"--device {args.device}: cuda or cpu")
    if args.min_views < 1 or not 0 <= args.min_percent <= 100 or args.dilate < 0 or args.max_points < 1 or not 1 <= args.grid <= carve.MAX_DIM:
        _fail(f"--min_views >= 1, 0 <= --min_percent <= 100, --dilate >= 0, --max_points >= 1 and 1 <= --grid <= {carve.MAX_DIM} expected")
    if args.directions and (args.rounds < 0 or not 0 <= args.min_conf <= 255 or not 0.0 < args.sigma_deg < 180.0):
        _fail("--rounds >= 0, 0 <= --min_conf <= 255 and 0 < --sigma_deg < 180 expected")
    if args.visibility:
        from utils import visibility
        if not args.directions:
            _fail("--visibility gates the votes of --directions: pass both")
        if args.mode == "filter":
            _fail("--visibility marches the carved grid, and --mode filter carves none: use --mode hull or both")
        if not 0 <= args.vis_skip <= visibility.MAX_SKIP or not 0 <= args.vis_max_blocked <= visibility.MAX_BLOCKED:
            _fail(f"0 <= --vis_skip <= {visibility.MAX_SKIP} and 0 <= --vis_max_blocked <= {visibility.MAX_BLOCKED} expected")
    src = args.source_path
    sparse = os.path.join(src, "sparse", "0")
    if not os.path.isdir(os.path.join(src, capture.MASKS)):
        _fail(f"{src} has no masks/ folder: there is nothing to carve with")
    result = os.path.join(sparse, "points3D.bin")
    backup = next((os.path.join(sparse, b) for b in BACKUPS if os.path.exists(os.path.join(sparse, b))), None)
    original = None
    if backup is not None:
        if os.path.exists(result) and not args.overwrite:
            _fail(f"{result} is the result of an earlier run (COLMAP's points are in {os.path.basename(backup)}): pass --overwrite")
    else:
        original = next((os.path.join(sparse, n) for n in ("points3D.bin", "points3D.txt") if os.path.exists(os.path.join(sparse, n))), None)
    need_images = args.mode in ("hull", "both")
    orients = confs = None
    try:
        views = load_views(sparse)
        masks = [read_plane(capture.mask_path(src, capture.file_name(v)), v, "the mask") for v in views]
        imgs = [read_plane(os.path.join(src, args.images, capture.file_name(v)), v, "the image", "RGB") for v in views] if need_images else None
        if args.directions:
            pairs = [capture.pair_paths(os.path.join(src, args.orientations), capture.file_name(v)) for v in views]
            orients = [read_plane(pair[0], v, "the orientation map") for pair, v in zip(pairs, views)]
            confs = [read_plane(pair[1], v, "the confidence map") for pair, v in zip(pairs, views)]
    except ValueError as e:
        _fail(str(e))
    voter = _Voter(views, masks, imgs, None if args.device == "cpu" else "cuda", args.dilate)
    parts, grid = [], None
    if args.mode in ("filter", "both"):
        source = backup or original
        if source is None:
            _fail(f"{sparse} holds no points3D.bin or points3D.txt to filter")
        xyz, rgb, err = (read_points3D_binary if source.endswith(".bin") else read_points3D_text)(source)
        seen, hits = voter.votes(xyz, False)[:2] if xyz.shape[0] else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        k = carve.keep(seen, hits, args.min_views, args.min_percent)
        print(f"filter: {int(k.sum())} of {xyz.shape[0]} COLMAP point(s) kept")
        parts.append((xyz[k], rgb[k].astype(np.uint8), err.reshape(-1)[k]))
    if args.mode in ("hull", "both"):
        xyz, rgb, grid = hull_points(voter, args)
        parts.append((xyz, rgb, np.zeros(xyz.shape[0], np.float64)))
    xyz, rgb, err = (np.concatenate([p[i] for p in parts]) for i in range(3))
    tmp = f"{result}.{os.getpid()}.tmp"
    n = write_points3D_arrays(xyz, rgb, err, tmp)
    if backup is None:                                       # the first run: COLMAP's points move aside, once
        if original is not None:
            os.replace(original, os.path.join(sparse, BACKUPS[0] if original.endswith(".bin") else BACKUPS[1]))
        else:
            write_points3D_arrays(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), np.zeros(0), os.path.join(sparse, BACKUPS[0]))
    os.replace(tmp, result)
    ply = os.path.join(sparse, "points3D.ply")               # (the loader's conversion of the old points)
    if os.path.exists(ply):
        os.remove(ply)
    print(f"{n} point(s) written to {result}")
    if args.directions:
        from data.dataset_readers import storePly
        normals, coherence = lift_normals(voter, orients, confs, xyz, args, grid if args.visibility else None)
        has = (normals != 0.0).any(axis=1)
        tmp = f"{ply}.{os.getpid()}.tmp"                         # (under a private name and renamed, as the loader writes it)
        storePly(tmp, xyz, rgb, normals)
        os.replace(tmp, ply)
        print(f"directions: {int(has.sum())} of {n} point(s) got one, median coherence "
              f"{float(np.median(coherence[has])) if has.any() else 0.0:.3f}; written to {ply}")
    return n


if __name__ == "__main__":
    main()
