"""Data loading and scene writing of the dataset synthesis without a GPU: the USC-HairSalon and Cem Yuksel strand loaders, OpenCV's
HSV2RGB, the evaluation file round trip, the OBJ reader, the point-cloud normals, and synthesize.py --device cpu end to end."""
import os

import numpy as np
import pytest

from tests.synth_fixtures import sphere_mesh, write_obj, write_usc


def test_usc_loader(tmp_path):
    from data.hair_data import USC_PALETTE, load_hair_from_usc_dataset
    walks = write_usc(str(tmp_path / "s.data"), n_long=100, seed=1)
    h = load_hair_from_usc_dataset(str(tmp_path / "s.data"), hsv_spectre_color=False, pct_strands=1)
    assert h.verts.shape == (100 * 100, 3) and h.edges.shape == (100 * 99, 2) and h.normals is None
    assert np.array_equal(h.verts, walks.reshape(-1, 3).astype(np.float64))
    assert np.array_equal(h.strand_root_idx, np.arange(100) * 100)
    assert np.array_equal(h.verts_id_to_strand_id, np.repeat(np.arange(100), 100))
    assert np.array_equal(h.edges[:2], [[0, 1], [1, 2]]) and h.edges.dtype == np.uint32
    # strand i (file position 100 k) takes palette[i % 3]
    assert np.array_equal(h.colors[100], USC_PALETTE[100 % 3]) and np.array_equal(h.colors[200], USC_PALETTE[200 % 3])
    h2 = load_hair_from_usc_dataset(str(tmp_path / "s.data"), hsv_spectre_color=True, pct_strands=1, normal_required=True)
    assert np.array_equal(h2.colors[0], [1, 0, 0, 1]) and h2.normals.shape == h2.verts.shape
    bad = tmp_path / "bad.data"
    bad.write_bytes(np.array([5], "<i4").tobytes())
    with pytest.raises(AssertionError):
        load_hair_from_usc_dataset(str(bad), pct_strands=100)


def test_cy_loader(tmp_path):
    from data.cy_hair import read_cy_hair, write_cy_hair
    from data.hair_data import CY_PALETTE, load_hair_from_cy_dataset
    rng = np.random.default_rng(0)
    segs = np.array([4, 6, 5, 3])                         # taken as POINT counts per strand, as the reference does
    pts = rng.normal(size=(segs.sum(), 3)).astype(np.float32) * 10
    write_cy_hair(str(tmp_path / "h.hair"), pts, segments=segs, info="test")
    f = read_cy_hair(str(tmp_path / "h.hair"))
    assert f.header.hair_count == 4 and f.header.info == "test" and np.array_equal(f.points, pts) and f.colors is None
    h = load_hair_from_cy_dataset(str(tmp_path / "h.hair"), hsv_spectre_color=False, pct_strands=50)
    keep = np.concatenate([np.arange(0, 4), np.arange(10, 15)])          # strands 0 and 2
    R = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], float)              # R_y(-90) R_x(-90): (x, y, z) -> (y, z, x)
    assert np.allclose(h.verts, (R @ (0.25 * pts[keep].astype(np.float64) / 100).T).T, rtol=0, atol=1e-12)
    assert np.array_equal(h.strand_root_idx, [0, 4]) and h.edges.shape == (3 + 4, 2)
    assert np.array_equal(h.colors[0], CY_PALETTE[0]) and np.array_equal(h.colors[4], CY_PALETTE[2])
    d = pts[1] - pts[0]
    assert np.allclose(h.normals[0], d / np.linalg.norm(d)) and np.array_equal(h.normals[3], [0, 0, 1])


@pytest.mark.parametrize("hue,rgb", [(0, (255, 0, 0)), (30, (255, 255, 0)), (60, (0, 255, 0)), (90, (0, 255, 255)),
                                     (120, (0, 0, 255)), (150, (255, 0, 255)), (180, (255, 0, 0)), (15, (255, 128, 0))])
def test_hsv2rgb(hue, rgb):
    from data.hair_data import hsv2rgb_u8
    assert tuple(hsv2rgb_u8(hue)) == rgb


def test_eval_npz_round_trip(tmp_path):
    from data.eval_data import load_hair_eval_data_npz
    from data.hair_data import load_hair_from_usc_dataset, save_hair_eval_data_npz
    write_usc(str(tmp_path / "s.data"), n_long=20, seed=3, n_verts=100)
    h = load_hair_from_usc_dataset(str(tmp_path / "s.data"), hsv_spectre_color=False, pct_strands=1)
    save_hair_eval_data_npz(str(tmp_path / "e.npz"), h)
    e = load_hair_eval_data_npz(str(tmp_path / "e.npz"))
    assert np.array_equal(e.points, h.verts[h.edges[:, 0]])
    d = h.verts[h.edges[:, 1]] - h.verts[h.edges[:, 0]]
    assert np.allclose(e.directions, d / np.linalg.norm(d, axis=1, keepdims=True))
    assert np.array_equal(e.points_id_to_strand_id, np.repeat(np.arange(20), 99))
    assert e.edges.shape == (20 * 98, 2) and e.edges.max() == 20 * 99 - 1


def test_obj_reader(tmp_path):
    from data.head_data import load_head_from_usc_dataset, load_obj
    p = tmp_path / "m.obj"
    p.write_text("# quad and a triangle\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0 1.0\nvn 0 0 1\nvn 0 0 -1\nvt 0 0\n"
                 "f 1//1 2//1 3//1 4//1\nf -4/1/2 -2/1/2 -1/1/2\n")
    v, f, n = load_obj(str(p))
    assert v.dtype == np.float32 and v.shape == (4, 3) and n.shape == (2, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 3]]
    h = load_head_from_usc_dataset(str(p), normal_required=True)      # 2 normals for 3 faces and 4 vertices: estimated
    assert h.normals.shape == (4, 3) and np.allclose(np.abs(h.normals[:, 2]), 1)
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1 2 3\n")      # one normal per face
    h = load_head_from_usc_dataset(str(p), normal_required=True)
    assert np.array_equal(h.normals, np.tile([0, 0, 1.0], (3, 1))) and h.colors.shape == (3, 4)


def test_normals_match_brute_force():
    from utils.normals import estimate_pointcloud_normals
    rng = np.random.default_rng(1)
    u = rng.uniform(-1, 1, (400, 2))
    pts = np.column_stack([u, 0.2 * u[:, 0] ** 2 + 0.1 * u[:, 1] + 0.01 * rng.normal(size=400)])
    got = estimate_pointcloud_normals(pts, neighborhood_size=50)
    d = ((pts[:, None] - pts[None]) ** 2).sum(-1)
    nb = np.argsort(d, axis=1, kind="stable")[:, :50]
    for i in range(0, 400, 7):
        q = pts[nb[i]]
        b = q - q.mean(0)
        w, V = np.linalg.eigh(b.T @ b / 50)
        n = V[:, 0]
        if ((q - pts[i]) @ n > 0).sum() < 25:
            n = -n
        assert np.allclose(got[i], n, atol=1e-9), i


def test_synthesize_cpu_scene_loads(tmp_path):
    import synthesize
    from PIL import Image
    from data.dataset_readers import readColmapSceneInfo
    from scene.scene import camera_from_info
    write_usc(str(tmp_path / "s.data"), n_long=1000, seed=4)
    v, f, n = sphere_mesh()
    write_obj(str(tmp_path / "head.obj"), v, f, n)
    out = tmp_path / "scene"
    argv = ["--dataset", "usc_hair_salon", "--hair", str(tmp_path / "s.data"), "--head", str(tmp_path / "head.obj"), "-o", str(out),
            "--pct_strands", "10", "--cameras", "4", "--width", "96", "--height", "64", "--cam_z", "0.45", "--device", "cpu"]
    assert synthesize.main(argv) == 0
    with pytest.raises(SystemExit):
        synthesize.main(argv)                                  # an existing folder is refused without --overwrite
    synthesize.main(argv + ["--overwrite"])
    for k in range(1, 5):
        img = np.asarray(Image.open(out / "images" / f"image_{k}.png"))
        mask = np.asarray(Image.open(out / "masks" / f"image_{k}.png"))
        assert img.shape == (64, 96, 3) and mask.shape == (64, 96) and set(np.unique(mask)) <= {0, 255}
        assert mask.any() and (img[mask > 0] != 0).any(axis=1).all()
        assert (out / "orientations" / f"image_{k}_orientation.png").exists()
    info = readColmapSceneInfo(str(out))                       # what Scene reads (Scene itself builds its model on the GPU)
    cams = [camera_from_info(k, c, data_device="cpu") for k, c in enumerate(info.cameras)]
    assert len(cams) == 4 and info.point_cloud.points.shape[0] == v.shape[0] and all(c.mask is not None and c.orientation_field is not None for c in cams)
    assert os.path.exists(out / "hair_eval_data.npz") and os.path.exists(out / "head_reconstruction_data.npz")
