"""A capture on disk (hair-gs_amd/data/capture.py) without a GPU: the scene-rewriting drivers refuse in their own name, the library
refuses with ValueError only, the names it forms are the ones orient.py writes and the loader finds, and no library module imports a
driver."""
import ast
import os

import numpy as np
import pytest

from tests import rescale_cases as RC
from tests import undistort_cases as UC

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hair-gs_amd")
DRIVERS = sorted(f[:-3] for f in os.listdir(PKG) if f.endswith(".py"))
PACKAGES = sorted(d for d in os.listdir(PKG) if os.path.isfile(os.path.join(PKG, d, "__init__.py")))

# view_1.png of both builders' scenes: camera 1, 48 x 36, with a mask
FAULTS = {"mask": r"masks/view_1\.png: a mask of 64 x 10 pixels, camera 1 has 48 x 36",
          "palette": r"images/view_1\.png: image mode P is not supported \(L, RGB or RGBA\)",
          "tiff": r"images/view_1\.png: format TIFF is not supported \(PNG or JPEG\)"}


def _spoil(src, fault):
    """Returns the spoilt file."""
    from PIL import Image as PILImage
    image, mask = os.path.join(src, "images", "view_1.png"), os.path.join(src, "masks", "view_1.png")
    if fault == "mask":
        PILImage.fromarray(np.zeros((10, 64), np.uint8)).save(mask)
        return mask
    with PILImage.open(image) as im:
        im = im.convert("P") if fault == "palette" else im.copy()
    im.save(image, format="TIFF" if fault == "tiff" else "PNG")
    return image


def _driver(name):
    if name == "rescale":
        import rescale
        return RC.build_scene, lambda src, out: rescale.main(["-s", src, "-o", out, "--device", "cpu", "-r", "2"])
    import undistort
    return UC.build_scene, lambda src, out: undistort.main(["-s", src, "-o", out, "--device", "cpu"])


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", ["rescale", "undistort"])
def test_driver_refuses_a_bad_file_in_its_own_name(tmp_path, name, fault):
    build, run = _driver(name)
    src = str(tmp_path / "src")
    build(src)
    _spoil(src, fault)
    with pytest.raises(SystemExit, match=rf"^{name}\.py: .*{FAULTS[fault]}$"):
        run(src, str(tmp_path / "out"))


@pytest.mark.parametrize("fault", list(FAULTS))
def test_library_reader_refuses_with_value_error(tmp_path, fault):
    from data import capture
    src = str(tmp_path / "src")
    RC.build_scene(src)
    path = _spoil(src, fault)
    with pytest.raises(ValueError, match=FAULTS[fault]):
        capture.read_image(path, (48, 36), "a mask" if fault == "mask" else "an image", "camera 1", convert="L" if fault == "mask" else None)
    with pytest.raises(ValueError, match=r"nowhere\.png is missing \(the mask of view 7\)$"):
        capture.read_image(str(tmp_path / "nowhere.png"), (48, 36), "a mask", "camera 1", of="the mask of view 7")


def test_library_raises_no_system_exit(tmp_path):
    from data import capture
    sparse = tmp_path / "sparse" / "0"
    sparse.mkdir(parents=True)
    (sparse / "cameras.txt").write_text("1 SIMPLE_RADIAL wide 36 40.0 24.0 18.0 0.1\n")
    (sparse / "images.txt").write_text("")
    with pytest.raises(ValueError, match="wide"):
        capture.read_sparse(str(sparse))
    with open(capture.__file__) as fh:
        assert "SystemExit" not in fh.read()


def test_layout_agrees_with_orient_and_the_loader(tmp_path):
    """Names with a second dot and with a folder in the model: the pairs orient.py writes and the planes the loader finds are at
    capture.pair_paths / mask_path of capture.file_name, and a camera is called capture.stem of it."""
    import shutil
    import orient
    from PIL import Image as PILImage
    from data import capture
    from data.colmap import write_images_binary
    from data.dataset_readers import readColmapSceneInfo
    src = str(tmp_path / "src")
    _, images = RC.build_scene(src)
    shutil.rmtree(os.path.join(src, "orientations"))
    renamed = {"view_1.png": "a.b.png", "view_2.jpg": "dir/x.jpg"}
    for old, new in renamed.items():
        for folder in ("images", "masks"):
            if os.path.exists(os.path.join(src, folder, old)):
                os.replace(os.path.join(src, folder, old), os.path.join(src, folder, os.path.basename(new)))
    images = {k: im._replace(name=renamed.get(im.name, im.name)) for k, im in images.items()}
    write_images_binary(images, os.path.join(src, "sparse", "0", "images.bin"))
    names = [capture.file_name(im) for im in images.values()]
    assert names == ["a.b.png", "x.jpg", "view_3.png", "view_4.png"]
    assert [capture.stem(n) for n in names] == ["a", "x", "view_3", "view_4"]
    assert orient.main(["-s", src, "--device", "cpu"]) == 4
    folder = os.path.join(src, capture.ORIENTATIONS)
    pairs = {n: capture.pair_paths(folder, n) for n in names}
    assert sorted(os.listdir(folder)) == sorted(os.path.basename(p) for pair in pairs.values() for p in pair)
    cams = {c.image_name: c for c in readColmapSceneInfo(src).cameras}
    assert sorted(cams) == sorted(capture.stem(n) for n in names)
    for n in names:
        c = cams[capture.stem(n)]
        assert c.image_path == os.path.join(src, capture.IMAGES, n)
        assert (c.mask is not None) == os.path.exists(capture.mask_path(src, n)) == (n in ("a.b.png", "view_3.png"))
        field, conf = (np.asarray(PILImage.open(p)).astype(np.float32) for p in pairs[n])
        assert np.array_equal(c.orientation_field, field * np.pi / 255.0) and np.array_equal(c.orientation_confidence, conf / 255.0)


# ---- who imports whom ------------------------------------------------------------------------------------------------------------
def _imports(path):
    """(tree, [(node, top-level module name)]) of every absolute import in a file."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            found += [(node, a.name.split(".")[0]) for a in node.names]
        elif isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
            found.append((node, node.module.split(".")[0]))
    return tree, found


@pytest.mark.parametrize("package", PACKAGES)
def test_no_library_module_imports_a_driver(package):
    """Every .py below hair-gs_amd/ that is no top-level driver, package by package."""
    assert "undistort" in DRIVERS and "train" in DRIVERS and "capture" not in DRIVERS
    bad = []
    for dp, _, fs in os.walk(os.path.join(PKG, package)):
        for f in sorted(fs):
            if f.endswith(".py"):
                bad += [f"{os.path.relpath(os.path.join(dp, f), PKG)}:{node.lineno} imports {mod}"
                        for node, mod in _imports(os.path.join(dp, f))[1] if mod in DRIVERS]
    assert not bad, bad


def test_a_driver_imports_another_only_to_run_it():
    """Among the top-level drivers: `import D` followed by D.main(...) and no other use of D; never `from D import helper`."""
    bad = []
    for d in DRIVERS:
        tree, found = _imports(os.path.join(PKG, d + ".py"))
        for node, mod in found:
            if mod not in DRIVERS:
                continue
            if isinstance(node, ast.ImportFrom):
                bad.append(f"{d}.py:{node.lineno} takes a helper from {mod}")
                continue
            alias = next(a.asname or a.name for a in node.names if a.name.split(".")[0] == mod)
            uses = [n for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == alias]
            calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and n.func in uses and n.func.attr == "main"]
            if not calls or any(u.attr != "main" for u in uses):
                bad.append(f"{d}.py:{node.lineno} imports {mod} for something other than running its main")
    assert not bad, bad
