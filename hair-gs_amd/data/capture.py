"""A capture on disk: where its files are, how they are named, how an image that belongs to a camera is read and written, and the
steps that write one scene from another.  The loader (data/dataset_readers.py) and every capture tool (orient.py, synthesize.py,
undistort.py, rescale.py, init_cloud.py, init_scalp.py) form their paths here, so that what one writes the others find.
  <scene>/sparse/0/{cameras,images,points3D}.{bin,txt}      read_sparse
  <scene>/<images>/<name>     <scene>/masks/<name>           name = file_name(image): the basename of the model's image name
  <scene>/orientations/<stem>_orientation.png, <stem>_confidence.png        stem(name): the name up to its first dot
Nothing here names a program or ends one: a refusal is a ValueError, and the driver that called says who refuses.  PIL is imported
where it is used, as the drivers do (a tool that only reads the sparse model needs none of it).
The scene-rewriting steps are what undistort.py and rescale.py share: check_output, view_jobs, write_sparse, process_folder.  Each
driver calls them in its own order, with its own cameras, keypoint rule and kernel."""
import os
import shutil

import numpy as np

IMAGES, MASKS, ORIENTATIONS = "images", "masks", "orientations"
ORIENTATION, CONFIDENCE = "_orientation.png", "_confidence.png"
FORMATS = ("PNG", "JPEG")
MODES = ("L", "RGB", "RGBA")


def read_sparse(sparse_dir):
    """(cameras, images) of a sparse model: binary if images.bin exists, else text (any camera model)."""
    from data.colmap import read_extrinsics_binary, read_extrinsics_text, read_intrinsics_binary, read_intrinsics_text
    if os.path.exists(os.path.join(sparse_dir, "images.bin")):
        return read_intrinsics_binary(os.path.join(sparse_dir, "cameras.bin")), read_extrinsics_binary(os.path.join(sparse_dir, "images.bin"))
    return (read_intrinsics_text(os.path.join(sparse_dir, "cameras.txt"), pinhole_only=False),
            read_extrinsics_text(os.path.join(sparse_dir, "images.txt")))


# ---- the layout ------------------------------------------------------------------------------------------------------
def file_name(image):
    """The file name, in <images>/ and masks/, of a model image (or of anything else with its .name, such as a utils.views View)."""
    return os.path.basename(image.name)


def stem(name):
    """What names a file's orientation pair, and its camera after loading: "a.b.png" -> "a"."""
    return name.split(".")[0]


def mask_path(scene, name):
    return os.path.join(scene, MASKS, name)


def pair_paths(folder, name):
    """(orientation map, confidence map) of the file `name`, in `folder`."""
    return os.path.join(folder, stem(name) + ORIENTATION), os.path.join(folder, stem(name) + CONFIDENCE)


# ---- images of a camera's size ---------------------------------------------------------------------------------------
def read_image(path, size, what, owner, convert=None, formats=FORMATS, of=None):
    """(uint8 [H, W] or [H, W, C] as PIL hands it out, read-only; its PIL format) of an image that must be size = (W, H), its
    camera's.  convert: a PIL mode to convert to first; formats: the accepted PIL formats, None for any.  `what` ("a mask") and
    `owner` ("camera 3") word the size refusal, `of` ("the mask of view x.png") says whose file is missing."""
    from PIL import Image
    if not os.path.exists(path):
        raise ValueError(f"{path} is missing" + (f" ({of})" if of else ""))
    with Image.open(path) as im:
        fmt = im.format
        if formats is not None and fmt not in formats:
            raise ValueError(f"{path}: format {fmt} is not supported (PNG or JPEG)")
        if convert is not None:
            im = im.convert(convert)
        if im.mode not in MODES:
            raise ValueError(f"{path}: image mode {im.mode} is not supported (L, RGB or RGBA)")
        a = np.asarray(im)
    if a.shape[:2] != (size[1], size[0]):
        raise ValueError(f"{path}: {what} of {a.shape[1]} x {a.shape[0]} pixels, {owner} has {size[0]} x {size[1]}")
    return a, fmt


def write_image(path, a, fmt):
    """a: uint8 [H, W, C]; a JPEG at quality 95, anything else as PNG."""
    from PIL import Image
    im = Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)
    if fmt == "JPEG":
        im.save(path, format="JPEG", quality=95)
    else:
        im.save(path, format="PNG")


# ---- one scene written from another ----------------------------------------------------------------------------------
def check_output(src, out, overwrite):
    if os.path.abspath(out) == os.path.abspath(src):
        raise ValueError("the output scene must not be the source scene")
    if os.path.isdir(out) and os.listdir(out) and not overwrite:
        raise ValueError(f"{out} exists and is not empty (pass --overwrite)")


def view_jobs(src, out, images_folder, images):
    """Yields (file name, image job, mask job or None) per model image, in the model's order; a job is (camera id, source path,
    output path).  An image file that is missing is refused when its turn comes."""
    for im in images.values():
        name = file_name(im)
        path = os.path.join(src, images_folder, name)
        if not os.path.exists(path):
            raise ValueError(f"{path} is missing")
        mask = mask_path(src, name)
        yield name, (im.camera_id, path, os.path.join(out, IMAGES, name)), \
            (im.camera_id, mask, mask_path(out, name)) if os.path.exists(mask) else None


def write_sparse(src, out, cameras, images, out_cameras, keypoints):
    """Makes <out>/sparse/0 and <out>/images and writes the model: out_cameras, the images with xys = keypoints(xys, camera,
    out_camera), the source's points3D.bin (or .txt) byte for byte; an earlier run's points3D.ply goes."""
    from data.colmap import write_cameras_binary, write_images_binary
    sparse, out_sparse = os.path.join(src, "sparse", "0"), os.path.join(out, "sparse", "0")
    for d in (out_sparse, os.path.join(out, IMAGES)):
        os.makedirs(d, exist_ok=True)
    write_cameras_binary(out_cameras, os.path.join(out_sparse, "cameras.bin"))
    write_images_binary({k: im._replace(xys=keypoints(im.xys, cameras[im.camera_id], out_cameras[im.camera_id])) for k, im in images.items()},
                        os.path.join(out_sparse, "images.bin"))
    for name in ("points3D.bin", "points3D.txt"):
        if os.path.exists(os.path.join(sparse, name)):
            shutil.copyfile(os.path.join(sparse, name), os.path.join(out_sparse, name))
            break
    stale = os.path.join(out_sparse, "points3D.ply")     # (the loader's conversion of an earlier run's points)
    if os.path.exists(stale):
        os.remove(stale)


def batches(groups, batch):
    """(key, at most `batch` items) over a dict of lists, group after group."""
    for key, items in groups.items():
        for b0 in range(0, len(items), batch):
            yield key, items[b0:b0 + batch]


def process_folder(jobs, cameras, gray, batch, fn):
    """Reads every job's image (gray: as one L plane, a mask), groups them by (camera id, shape), hands fn(camera id, uint8
    [B, H, W, C]) at most `batch` of a group at a time and writes what it returns, [B, H', W', C], in each source's format."""
    groups = {}
    for cid, src, dst in jobs:
        cam = cameras[cid]
        a, fmt = read_image(src, (int(cam.width), int(cam.height)), "a mask" if gray else "an image", f"camera {cam.id}",
                            convert="L" if gray else None)
        a = a.reshape(a.shape[0], a.shape[1], -1)
        groups.setdefault((cid, a.shape), []).append((a, fmt, dst))
    for (cid, _), chunk in batches(groups, batch):
        out = fn(cid, np.stack([a for a, _, _ in chunk]))
        for i, (_, fmt, dst) in enumerate(chunk):
            write_image(dst, out[i], fmt)
    return len(jobs)
