#!/usr/bin/env python3
"""Synthesizes a multi-view capture from a strand file and a head mesh, as the reference's dataset scripts do
(scripts/parse_usc_hairsalon.py, scripts/download_parse_cy.py), with the rasterizer of scene/mesh_renderer.py in place of OpenGL.
  python synthesize.py --dataset usc_hair_salon|cem_yuksel --hair <strands file> --head <obj> -o <scene>
      [--pct_strands 100] [--line_width 1] [--hsv] [--cam_z (0.5 usc / 0.3 cy)] [--cameras 16] [--height 1000] [--width 1000]
      [--use_gt_hair_verts | --use_strand_root_verts] [--device cuda|cpu] [--normals host|device] [--batch 16] [--overwrite]
Writes <scene>/images/image_<id>.png (the lit head and the hair), masks/image_<id>.png (255 where the render of the black head and
the hair is not black), orientations/image_<id>_{orientation,confidence}.png (utils.vision, as orient.py writes them; the paths are data/capture.py's),
hair_eval_data.npz, head_reconstruction_data.npz and sparse/0/{cameras,images,points3D}.bin.  The models are [black unlit head,
lit head (ka = kd = 0.5), lit hair], lit from (0, 5, 5) in white; the cameras ring the hair at its mid-height.  On the GPU the
images, masks and orientation maps of a batch stay on the device until the PNGs are written.  An existing output folder is
refused unless --overwrite is given.  --normals device estimates the hair's (and, where the head file has none, the head's) vertex
normals with the HIP kernels of utils.normals instead of the host's k-d tree (needs --device cuda; same contract, last-place
differences: the default stays host so that existing captures keep their bytes)."""
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np


def build_models(hair, head, line_width):
    from scene.mesh_renderer import MeshModel
    black = MeshModel(head.verts, faces=head.faces, colors=np.zeros_like(head.colors), normals=head.normals, use_lighting=False)
    lit = MeshModel(head.verts, faces=head.faces, colors=head.colors, normals=head.normals, use_lighting=True, ka=0.5, kd=0.5)
    strands = MeshModel(hair.verts, edges=hair.edges, colors=hair.colors, normals=hair.normals, use_lighting=True,
                        line_width=line_width, ka=0.5, kd=0.5)
    return [black, lit, strands]


def lighting():
    from scene.mesh_renderer import Lighting
    return Lighting(light_pos=np.array([0, 5, 5]), ambient_color=np.array([1, 1, 1, 1]), diffuse_color=np.array([1, 1, 1, 1]))


def ring_cameras(hair, n, height, width, cam_z):
    """COLMAP cameras and world-to-camera matrices around the hair (the reference's pose: camera 1 at (0, mid-height, cam_z)
    looking down -z in OpenCV axes, the ring about the y axis through (0, mid-height, 0), the last camera above)."""
    from utils.camera import generate_cameras
    cam_pose = np.eye(4)
    cam_y = (hair.verts[:, 1].max() + hair.verts[:, 1].min()) / 2
    cam_pose[:3, 3] = [0, cam_y, cam_z]
    cam_pose[:3, 1:3] *= -1
    return generate_cameras(n, height, width, cam_pose=cam_pose, anchor_pos=np.array([0, cam_y, 0]), offset=cam_z)


def camera_matrices(cams, Es):
    from utils.camera import colmap_camera_to_projection_matrix, opencv_to_opengl_view_matrix
    ids = list(cams.keys())
    views = np.stack([opencv_to_opengl_view_matrix(Es[i]) for i in ids])
    projs = np.stack([colmap_camera_to_projection_matrix(cams[i]) for i in ids])
    return ids, views, projs


def _save(path, arr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


def render_capture(models, light, ids, views, projs, width, height, device, batch, out):
    """Renders and writes images, masks and orientation maps; returns the dropped primitive count of all renders."""
    from data import capture
    from scene.mesh_renderer import render_views
    from utils.vision import estimate_orientation_field, estimate_orientation_fields, orientation_pngs
    images, orientations = os.path.join(out, capture.IMAGES), os.path.join(out, capture.ORIENTATIONS)
    for d in (images, os.path.join(out, capture.MASKS), orientations):
        os.makedirs(d, exist_ok=True)
    dropped = 0
    state = {}
    on_gpu = device is not None and str(device) != "cpu"
    if on_gpu:
        from scene._raster_device import DeviceMeshes
        from scene.mesh_renderer import _Prepared
        state = {k: DeviceMeshes(_Prepared(models, list(k)), device) for k in ((1, 2), (0, 2))}
    for b0 in range(0, len(ids), max(1, batch)):
        sl = slice(b0, b0 + max(1, batch))
        kw = dict(lighting=light, device=device)
        img, d1, gray = render_views(models, views[sl], projs[sl], width, height, mesh_indices=[1, 2], return_gray=True,
                                     _device_state=state.get((1, 2)), **kw)
        msk, d2 = render_views(models, views[sl], projs[sl], width, height, mesh_indices=[0, 2], _device_state=state.get((0, 2)), **kw)
        dropped += d1 + d2
        if on_gpu:
            import torch
            mask = (msk != 0).any(dim=3).to(torch.uint8) * 255
            field, conf = estimate_orientation_fields(gray)
            img, mask, field, conf = img.cpu().numpy(), mask.cpu().numpy(), field.cpu().numpy(), conf.cpu().numpy()
        else:
            mask = (msk != 0).any(axis=3).astype(np.uint8) * 255
            fc = [estimate_orientation_field(g) for g in gray]
            field, conf = np.stack([f for f, _ in fc]), np.stack([c for _, c in fc])
        for k, cid in enumerate(ids[sl]):
            name = f"image_{cid}.png"                            # (the name data.colmap.generate_colmap_data gives the view)
            _save(os.path.join(images, name), img[k])
            _save(capture.mask_path(out, name), mask[k])
            for path, plane in zip(capture.pair_paths(orientations, name), orientation_pngs(field[k], conf[k])):
                _save(path, plane)
    return dropped


def main(argv=None):
    parser = ArgumentParser(description="Synthesize a multi-view capture from a strand file and a head mesh")
    parser.add_argument("--dataset", required=True, choices=["usc_hair_salon", "cem_yuksel"])
    parser.add_argument("--hair", required=True, help="USC-HairSalon .data or Cem Yuksel .hair file")
    parser.add_argument("--head", required=True, help="head mesh (.obj)")
    parser.add_argument("--output", "-o", required=True, help="scene directory to write")
    parser.add_argument("--pct_strands", "-p", type=float, default=100, help="percentage of the strands to keep")
    parser.add_argument("--line_width", "-w", type=float, default=1, help="width of the rendered lines (pixels)")
    parser.add_argument("--hsv", action="store_true", help="one hue per strand instead of the palette")
    parser.add_argument("--cam_z", type=float, default=None, help="camera distance (default 0.5 usc_hair_salon, 0.3 cem_yuksel)")
    parser.add_argument("--cameras", type=int, default=16)
    parser.add_argument("--height", type=int, default=1000)
    parser.add_argument("--width", type=int, default=1000)
    init = parser.add_mutually_exclusive_group()
    init.add_argument("--use_gt_hair_verts", action="store_true", help="initial point cloud: the hair vertices")
    init.add_argument("--use_strand_root_verts", action="store_true", help="initial point cloud: the strand roots")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the CPU path")
    parser.add_argument("--normals", default="host", choices=["host", "device"],
                        help="vertex normals: host = scipy k-d tree + LAPACK; device = the HIP kernels (needs --device cuda)")
    parser.add_argument("--batch", type=int, default=16, help="views per render call")
    parser.add_argument("--overwrite", action="store_true", help="replace an existing output folder")
    args = parser.parse_args(argv)
    if args.normals == "device" and args.device == "cpu":
        parser.error("--normals device needs a GPU: it cannot be combined with --device cpu")
    from data.colmap import generate_colmap_data, write_cameras_binary, write_images_binary, write_points3D_binary
    from data.hair_data import hair_data_load_callbacks, save_hair_eval_data_npz
    from data.head_data import head_data_load_callbacks
    from data.head_reconstruction_data import save_head_reconstruction_data_npz
    out = args.output
    if os.path.exists(out):
        if not args.overwrite:
            raise SystemExit(f"synthesize.py: {out} exists (--overwrite replaces it)")
        shutil.rmtree(out)
    device = None if args.device == "cpu" else args.device
    normals_device = args.device if args.normals == "device" else None
    cam_z = args.cam_z if args.cam_z is not None else (0.5 if args.dataset == "usc_hair_salon" else 0.3)
    t0 = time.time()
    if args.dataset == "usc_hair_salon":
        head = head_data_load_callbacks["usc_hair_salon"](args.head, normal_required=True, normals_device=normals_device)
        hair = hair_data_load_callbacks["usc_hair_salon"](args.hair, normal_required=True, hsv_spectre_color=args.hsv,
                                                          pct_strands=args.pct_strands, normals_device=normals_device)
    else:
        head = head_data_load_callbacks["cem_yuksel"](args.head, normals_device=normals_device)
        hair = hair_data_load_callbacks["cem_yuksel"](args.hair, hsv_spectre_color=args.hsv, pct_strands=args.pct_strands)
    t1 = time.time()
    cams, Es = ring_cameras(hair, args.cameras, args.height, args.width, cam_z)
    ids, views, projs = camera_matrices(cams, Es)
    os.makedirs(out)
    dropped = render_capture(build_models(hair, head, args.line_width), lighting(), ids, views, projs, args.width, args.height, device,
                             args.batch, out)
    t2 = time.time()
    save_hair_eval_data_npz(os.path.join(out, "hair_eval_data.npz"), hair)
    save_head_reconstruction_data_npz(os.path.join(out, "head_reconstruction_data.npz"), head.verts, hair.verts[hair.strand_root_idx])
    if args.use_gt_hair_verts:
        points, colors = hair.verts, hair.colors
    elif args.use_strand_root_verts:
        points, colors = hair.verts[hair.strand_root_idx], hair.colors[hair.strand_root_idx]
    else:
        points, colors = head.verts, head.colors
    images, points3d = generate_colmap_data(cams, Es, points, colors)
    sparse = os.path.join(out, "sparse", "0")
    os.makedirs(sparse)
    write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    write_images_binary(images, os.path.join(sparse, "images.bin"))
    write_points3D_binary(points3d, os.path.join(sparse, "points3D.bin"))
    print(f"synthesize.py: {len(ids)} views of {hair.edges.shape[0]} segments and {head.faces.shape[0]} triangles -> {out} "
          f"(load {t1 - t0:.1f} s, render + orientation {t2 - t1:.1f} s, {dropped} dropped primitive(s), "
          f"normals: {args.normals})")
    return dropped


if __name__ == "__main__":
    main()
