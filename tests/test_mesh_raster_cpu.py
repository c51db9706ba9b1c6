"""The rasterizer of the dataset synthesis without a GPU (hair-gs_amd/scene/mesh_renderer.py): hand-derived line and triangle
coverage, the draw-order tie rule, dropped primitives, the camera matrices, and the agreement of a synthesized capture's images
with the cameras the trainer loads from its sparse model."""
import os

import numpy as np
import pytest

I4 = np.eye(4)


def _ndc(i, j, W, H):
    """NDC of window position (i, j) in pixels (pixel centres at i + 0.5), under identity view and projection."""
    return (i / W) * 2 - 1, (j / H) * 2 - 1


def _line(p, q, W, H, width=1.0, color=(1, 0, 0, 1), z=(0.0, 0.0)):
    from scene.mesh_renderer import MeshModel
    a, b = _ndc(*p, W, H), _ndc(*q, W, H)
    return MeshModel(np.array([[a[0], a[1], z[0]], [b[0], b[1], z[1]]]), colors=np.array(color), edges=np.array([[0, 1]]),
                     use_lighting=False, line_width=width)


def _cover(models, W, H, **kw):
    """bool [H_window, W]: pixels that are not background, indexed by WINDOW row (from the bottom)."""
    from scene.mesh_renderer import render_views
    img, dropped = render_views(models, I4, I4, W, H, **kw)
    return (img[0] != 0).any(axis=2)[::-1], dropped, img[0]


def test_horizontal_line_is_half_open():
    W, H = 8, 4
    cov, _, _ = _cover([_line((0.5, 1.5), (5.5, 1.5), W, H)], W, H)
    assert np.nonzero(cov[1])[0].tolist() == [0, 1, 2, 3, 4] and cov.sum() == 5
    cov, _, _ = _cover([_line((5.5, 1.5), (0.5, 1.5), W, H)], W, H)
    assert np.nonzero(cov[1])[0].tolist() == [1, 2, 3, 4, 5] and cov.sum() == 5


def test_diagonal_line_one_fragment_per_column():
    W, H = 8, 8
    cov, _, _ = _cover([_line((0.5, 0.5), (5.5, 5.5), W, H)], W, H)
    assert sorted(zip(*np.nonzero(cov))) == [(k, k) for k in range(5)]
    cov, _, _ = _cover([_line((0.5, 0.5), (2.5, 6.5), W, H)], W, H)        # y-major: one fragment per row
    rows = np.nonzero(cov)[0]
    assert sorted(rows.tolist()) == list(range(6))


@pytest.mark.parametrize("width,rows", [(1.0, [3]), (2.0, [3, 4]), (3.0, [2, 3, 4]), (3.5, [2, 3, 4, 5]), (0.2, [3])])
def test_wide_line_column(width, rows):
    W, H = 8, 8
    cov, _, _ = _cover([_line((0.5, 3.5), (6.5, 3.5), W, H, width=width)], W, H)
    assert np.nonzero(cov.any(axis=1))[0].tolist() == rows
    assert all(np.nonzero(cov[r])[0].tolist() == list(range(6)) for r in rows)


def _tri_model(pts_px, W, H, faces, z=0.0, color=(0, 1, 0, 1)):
    from scene.mesh_renderer import MeshModel
    v = np.array([[*_ndc(x, y, W, H), z] for x, y in pts_px])
    return MeshModel(v, faces=np.asarray(faces), colors=np.array(color), use_lighting=False)


def test_two_triangles_cover_a_square_once():
    W, H = 8, 8
    pts = [(1, 1), (5, 1), (5, 5), (1, 5)]                    # window corners on pixel boundaries: pixels 1..4 inside
    total = np.zeros((H, W), int)
    for f in ([0, 1, 2], [0, 2, 3]):
        cov, _, _ = _cover([_tri_model(pts, W, H, [f])], W, H)
        total += cov
    want = np.zeros((H, W), int)
    want[1:5, 1:5] = 1
    assert np.array_equal(total, want)
    pts = [(0.5, 0.5), (4.5, 0.5), (4.5, 4.5), (0.5, 4.5)]    # corners on pixel centres: the top-left rule splits the edges
    total = np.zeros((H, W), int)
    for f in ([0, 1, 2], [0, 2, 3]):
        cov, _, _ = _cover([_tri_model(pts, W, H, [f])], W, H)
        total += cov
    assert total.max() == 1 and total.sum() == 16


def test_clockwise_triangle_is_culled():
    W, H = 8, 8
    cov, dropped, _ = _cover([_tri_model([(1, 1), (6, 1), (1, 6)], W, H, [[0, 1, 2]])], W, H)
    assert cov.sum() > 0 and dropped == 0
    cov, dropped, _ = _cover([_tri_model([(1, 1), (6, 1), (1, 6)], W, H, [[0, 2, 1]])], W, H)
    assert cov.sum() == 0 and dropped == 0


def _uv_sphere(n_lat=24, n_lon=48, r=0.09, centre=(0, 0, 0)):
    """Closed sphere, counter-clockwise faces seen from outside."""
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.ones_like(lon)[None],
                     -np.sin(lat)[:, None] * np.sin(lon)[None]], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 1, 0]], ring, [[0, -1, 0]]]) * r + np.asarray(centre)
    f = []
    idx = lambda a, b: 1 + a * n_lon + (b % n_lon)
    for b in range(n_lon):
        f.append([0, idx(0, b), idx(0, b + 1)])
        f.append([len(v) - 1, idx(n_lat - 2, b + 1), idx(n_lat - 2, b)])
        for a in range(n_lat - 2):
            f.append([idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)])
            f.append([idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)])
    f = np.array(f)
    # orient every face outwards
    c = v[f].mean(1) - np.asarray(centre)
    nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    flip = (nrm * c).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f


def _persp(W, H, dist=0.3, f=None):
    from utils.camera import ColmapCamera, colmap_camera_to_projection_matrix, opencv_to_opengl_view_matrix
    cam = ColmapCamera(1, "SIMPLE_PINHOLE", W, H, [f or 1.2 * W, W / 2, H / 2])
    w2c = np.eye(4)
    w2c[:3, :3] = np.diag([1.0, -1.0, -1.0])          # OpenCV camera at +z looking down -z
    w2c[:3, 3] = [0, 0, dist]
    return opencv_to_opengl_view_matrix(w2c), colmap_camera_to_projection_matrix(cam)


def test_closed_sphere_covers_each_pixel_once():
    from scene import mesh_renderer as R
    W, H = 64, 48
    v, f = _uv_sphere()
    view, proj = _persp(W, H)
    counts = []
    for faces in (f, f[:, [0, 2, 1]]):                  # front faces, then the back faces (the same mesh turned inside out)
        m = R.MeshModel(v, faces=faces, use_lighting=False)
        prep = R._Prepared([m], None)
        vws, prj = R._check_views(view, proj)
        X, Y, z, cw, ok = R._vertex_stage(prep.pw, vws[0], prj[0], W, H)
        assert ok.all()
        pix, _ = R._triangles(X, Y, z, cw, ok, prep.idx.reshape(-1, 3), np.arange(len(faces)), W, H)
        counts.append(np.bincount(pix, minlength=W * H).reshape(H, W))
    front, back = counts
    assert front.max() == 1 and back.max() == 1
    assert np.array_equal(front, back)                 # inside the silhouette, once from each side
    assert 300 < front.sum() < W * H
    for row in front:                                  # no cracks: every row of the convex silhouette is one run
        on = np.nonzero(row)[0]
        assert on.size == 0 or on[-1] - on[0] + 1 == on.size


def test_first_model_in_list_order_wins_ties():
    W, H = 8, 4
    red = _line((0.5, 1.5), (6.5, 1.5), W, H, color=(1, 0, 0, 1), z=(1e-9, 1e-9))
    blue = _line((0.5, 1.5), (6.5, 1.5), W, H, color=(0, 0, 1, 1), z=(0.0, 0.0))
    for order in ([0, 1], [1, 0], None):
        _, _, img = _cover([red, blue], W, H, mesh_indices=order)
        assert (img[2, :6] == [255, 0, 0]).all(), order              # depths within one 24-bit step: the first draw keeps it
        _, _, img = _cover([blue, red], W, H, mesh_indices=order)
        assert (img[2, :6] == [0, 0, 255]).all(), order
    farther = _line((0.5, 1.5), (6.5, 1.5), W, H, color=(1, 0, 0, 1), z=(1e-3, 1e-3))
    _, _, img = _cover([farther, blue], W, H)
    assert (img[2, :6] == [0, 0, 255]).all()                          # a whole step nearer wins whatever the order
    _, _, img = _cover([farther, blue], W, H, mesh_indices=[0])
    assert (img[2, :6] == [255, 0, 0]).all()


def test_dropped_primitives_are_counted():
    from scene.mesh_renderer import MeshModel, render_views
    W, H = 32, 24
    view, proj = _persp(W, H)
    # camera at z = 0.3 looking down -z: z = 0.5 is behind it, z = -5 past the far plane (5 m from the camera)
    v = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0, 0.5], [0.01, 0.01, 0], [0, 0, -5], [0.02, 0, 0], [-0.01, 0.005, 0]])
    m = MeshModel(v, edges=np.array([[0, 1], [2, 3], [4, 5], [0, 6]]), use_lighting=False)
    img, dropped = render_views([m], view, proj, W, H)
    assert dropped == 2 and (img != 0).any()
    img, dropped = render_views([m, m], np.stack([view, view]), proj, W, H)
    assert dropped == 8 and img.shape == (2, H, W, 3)
    t = MeshModel(v, faces=np.array([[0, 1, 3], [0, 1, 2]]), use_lighting=False)
    assert render_views([t], view, proj, W, H)[1] == 1


def test_errors_before_any_work():
    from scene.mesh_renderer import MeshModel, render_views
    with pytest.raises(ValueError):
        render_views([], I4, I4, 8, 8)
    m = MeshModel(np.zeros((2, 3)), edges=np.array([[0, 1]]))
    with pytest.raises(IndexError):
        render_views([m], I4, I4, 8, 8, mesh_indices=[1])
    with pytest.raises(ValueError):
        MeshModel(np.zeros((3, 3)), edges=np.array([[0, 1]]), faces=np.array([[0, 1, 2]]))
    with pytest.raises(ValueError):
        MeshModel(np.zeros((3, 3)))


def test_model_defaults_follow_the_reference():
    from scene.mesh_renderer import MeshModel
    m = MeshModel(np.zeros((4, 3)), faces=np.array([[0, 1, 2]]), colors=np.array([0.1, 0.2, 0.3, 1]))
    assert m.colors.shape == (4, 4) and m.colors.dtype == np.float32 and (m.colors == np.float32(0.2))[:, 1].all()
    assert np.array_equal(m.normals, np.ones((4, 3), np.float32))
    assert (m.ka, m.kd, m.use_lighting, m.line_width) == (0.5, 0.5, True, 1.0)


def test_lit_shading_of_one_pixel():
    """A lit triangle facing the light: light = ka amb + kd cos dif, byte = floor(255 out + 0.5), computed here by hand."""
    from scene.mesh_renderer import Lighting, MeshModel, render_views
    W, H = 8, 8
    v = np.array([[*_ndc(x, y, W, H), 0.0] for x, y in [(0, 0), (8, 0), (0, 8)]])
    m = MeshModel(v, faces=np.array([[0, 1, 2]]), colors=np.array([0.8, 0.4, 0.2, 1]), normals=np.tile([0, 0, 1.0], (3, 1)),
                  ka=0.25, kd=0.5)
    light = Lighting(light_pos=np.array([0.0, 0.0, 10.0]), ambient_color=np.ones(4), diffuse_color=np.ones(4))
    img, _ = render_views([m], I4, I4, W, H, lighting=light)
    # the pixel with window centre (0.5, 0.5): position (-0.875, -0.875, 0)
    p = np.array([-0.875, -0.875, 0.0])
    d = np.array([0.0, 0.0, 10.0]) - p
    cos = d[2] / np.sqrt(d @ d)
    want = np.floor(np.clip((0.25 + 0.5 * cos) * np.float32([0.8, 0.4, 0.2]).astype(np.float64), 0, 1) * 255 + 0.5)
    assert np.array_equal(img[0, H - 1, 0], want.astype(np.uint8))


def test_projection_and_view_matrices():
    from utils.camera import ColmapCamera, colmap_camera_to_projection_matrix, opencv_to_opengl_view_matrix
    from utils.graphics import focal2fov
    cam = ColmapCamera(1, "SIMPLE_PINHOLE", 1000, 800, [500.0, 500.0, 400.0])
    P = colmap_camera_to_projection_matrix(cam)
    fovy, aspect, n, f = focal2fov(500.0, 800), 1000 / 800, 0.01, 5.0
    c = 1 / np.tan(fovy / 2)
    glu = np.array([[c / aspect, 0, 0, 0], [0, c, 0, 0], [0, 0, (f + n) / (n - f), 2 * f * n / (n - f)], [0, 0, -1, 0]])
    assert np.allclose(P, glu, rtol=1e-12, atol=1e-15)
    rng = np.random.default_rng(0)
    w2c = np.eye(4)
    w2c[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    w2c[:3, 3] = rng.normal(size=3)
    assert np.array_equal(opencv_to_opengl_view_matrix(w2c), np.diag([1.0, -1, -1, 1]) @ w2c)


def test_project_opencv_truncates_to_int16():
    from utils.camera import ColmapCamera, project_opencv
    cam = ColmapCamera(1, "SIMPLE_PINHOLE", 100, 80, [50.0, 50.0, 40.0])
    E = np.eye(4)
    uv = project_opencv(cam, E, np.array([[0.1, -0.1, 1.0], [-0.019, 0.0, 1.0]]))
    assert uv.dtype == np.int16 and uv.tolist() == [[55, 35], [49, 40]]


def test_images_agree_with_the_written_cameras(tmp_path):
    """The camera convention test: a capture written by generate_colmap_data and the writers, loaded back through
    readColmapSceneInfo and the trainer's Camera; the renderer's fragment of a short segment at a world point lies within 1 px of
    where the 3DGS camera (full_proj_transform, pixel centres at integers) projects the point."""
    import torch
    from PIL import Image
    from data.colmap import generate_colmap_data, write_cameras_binary, write_images_binary, write_points3D_binary
    from data.dataset_readers import readColmapSceneInfo
    from data.hair_data import HairData
    from scene.mesh_renderer import MeshModel, render_views
    from scene.scene import camera_from_info
    from synthesize import camera_matrices, ring_cameras
    W, H = 120, 90
    rng = np.random.default_rng(3)
    hair = HairData(verts=rng.uniform(-0.03, 0.03, (50, 3)), colors=None, normals=None, edges=None, strand_root_idx=None,
                    verts_id_to_strand_id=None)
    cams, Es = ring_cameras(hair, 5, H, W, 0.5)
    ids, views, projs = camera_matrices(cams, Es)
    images, pts = generate_colmap_data(cams, Es, hair.verts, np.ones((50, 4)) * 0.5)
    sparse = tmp_path / "sparse" / "0"
    os.makedirs(sparse)
    write_cameras_binary(cams, str(sparse / "cameras.bin"))
    write_images_binary(images, str(sparse / "images.bin"))
    write_points3D_binary(pts, str(sparse / "points3D.bin"))
    os.makedirs(tmp_path / "images")
    for cid in ids:
        Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(tmp_path / "images" / f"image_{cid}.png")
    info = readColmapSceneInfo(str(tmp_path))
    loaded = {c.image_name: camera_from_info(k, c, data_device="cpu") for k, c in enumerate(info.cameras)}
    worst = 0.0
    for p in rng.uniform(-0.025, 0.025, (12, 3)):
        for k, cid in enumerate(ids):
            cam = loaded[f"image_{cid}"]
            c2w = np.linalg.inv(Es[cid])
            depth = (Es[cid][:3, :3] @ p + Es[cid][:3, 3])[2]
            right = c2w[:3, 0] * depth / cams[cid].params[0]       # one pixel along the camera's x axis, starting at p
            m = MeshModel(np.stack([p, p + right]), edges=np.array([[0, 1]]), use_lighting=False)
            img, dropped = render_views([m], views[k], projs[k], W, H)
            ys, xs = np.nonzero((img[0] != 0).any(axis=2))
            if xs.size == 0:
                continue
            assert dropped == 0 and xs.size <= 2
            ph = torch.tensor([*p, 1.0], dtype=torch.float32) @ cam.full_proj_transform.cpu()
            ndc = (ph[:3] / ph[3]).numpy()
            u, v = ((ndc[0] + 1) * W - 1) * 0.5, ((ndc[1] + 1) * H - 1) * 0.5
            err = max(np.abs(xs - u).max(), np.abs(ys - v).max())
            worst = max(worst, err)
            assert err <= 1.0, (cid, p, xs, ys, u, v)
    print(f"largest pixel offset {worst:.3f}")
