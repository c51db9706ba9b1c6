"""The strand export on the CPU (scene/strand_export.py numpy path, data/strand_files.py, utils/ply.py lists, export_strands.py):
the vectorised path against the loop restatement of the contract (tests/strand_export_reference.py), native mode against the
evaluation points of the model, the filters on a hand-built model, every file format read back, and the driver."""
import os
import struct

import numpy as np
import pytest
import torch

from tests import strand_export_reference as R


@pytest.fixture(scope="module")
def mixed():
    return R.mixed_model([1, 2, 63, 64, 65, 130, 5, 17, 1, 130], seed=3)


@pytest.fixture(scope="module")
def collapsed():
    return R.collapsed_model(14, n_seg=12, seed=5)


@pytest.mark.parametrize("M", [2, 3, 64, 65, 100])
def test_numpy_path_matches_the_loop_restatement(mixed, M):
    from scene.strand_export import resample_strands
    res = resample_strands(mixed, points=M)
    ref = R.reference_export(mixed, M)
    R.assert_close(res, ref, mixed, what=f"mixed M={M}")
    assert np.array_equal(res.strand_ids, np.arange(10)) and res.points.shape[0] == 10 * M
    assert np.array_equal(res.length, ref[3])          # (both sum in segment order)
    # end samples are the end vertices, bit for bit
    offsets, rows, _, ep, _ = R.strand_tables(mixed)
    assert np.array_equal(res.points[res.offsets[:-1]], ep[rows[offsets[:-1], 0]])
    assert np.array_equal(res.points[res.offsets[1:] - 1], ep[rows[offsets[1:] - 1, 1]])


def test_attribute_table_is_colour_opacity_width(mixed):
    from scene.strand_export import ATTRIBUTES, export_attributes
    from utils.sh import C0
    t = export_attributes(mixed).numpy()
    assert t.dtype == np.float32 and t.shape == (mixed.endpoint_pairs.shape[0], len(ATTRIBUTES)) and len(ATTRIBUTES) == 5
    dc = mixed._features_dc.detach().numpy().reshape(-1, 3).astype(np.float64)
    want = np.concatenate([np.clip(0.5 + C0 * dc, 0, 1), 1 / (1 + np.exp(-mixed._opacity.detach().numpy().astype(np.float64))),
                           np.exp(mixed._width.detach().numpy().astype(np.float64))], axis=1)
    assert np.all(np.abs(t[:, :3] - want[:, :3]) <= 2 * R.EPS32)                          # (two float32 operations on values near 1)
    assert np.all(np.abs(t[:, 3:] - want[:, 3:]) <= 0.5 * R.EPS32 * np.abs(want[:, 3:]))  # the activations: float64 rounded once
    assert t[:, :3].min() == 0.0 and t[:, :3].max() == 1.0                                # (the clamp is exercised)
    # within a float32 unit of what the model renders with
    assert np.all(np.abs(t[:, 4] - mixed.get_scaling[:, 1].detach().numpy()) <= R.EPS32 * t[:, 4])
    assert np.all(np.abs(t[:, 3] - mixed.get_opacity[:, 0].detach().numpy()) <= R.EPS32 * t[:, 3])


@pytest.mark.parametrize("M", [2, 3, 65, 100])
def test_collapsed_segments(collapsed, M):
    from scene.strand_export import resample_strands
    m, has = collapsed
    S = has.shape[0]
    # attributes are discontinuous across a zero-length segment: compared on the strands without one, the other 5 of 7
    assert np.array_equal(has, np.isin(np.arange(S) % 7, (1, 2))) and (~has).sum() * 7 == 5 * S
    res = resample_strands(m, points=M)
    ref = R.reference_export(m, M)
    R.assert_close(res, ref, m, attr_strands=set(np.nonzero(~has)[0].tolist()), what=f"collapsed M={M}")
    # the strand that is one point: M copies of it, length 0
    assert res.length[2] == 0.0 and np.all(res.points[2 * M:3 * M] == res.points[2 * M])


def test_native_mode_is_the_joints_and_the_eval_points(mixed, tmp_path):
    from data.eval_data import load_hair_eval_data_npz
    from data.strand_files import strand_eval_data, write_strands_npz
    from loss.metrics import compute_eval_data_from_hair_gs
    from scene.strand_export import resample_strands
    res = resample_strands(mixed, points=0)
    ref = R.reference_export(mixed, 0)
    R.assert_close(res, ref, mixed, what="native")
    offsets, rows, _, ep, _ = R.strand_tables(mixed)
    n = offsets[1:] - offsets[:-1]
    assert np.array_equal(res.offsets, np.concatenate([[0], np.cumsum(n + 1)]))
    for s in range(len(n)):
        ids = np.concatenate([rows[offsets[s]:offsets[s + 1], 0], rows[offsets[s + 1] - 1:offsets[s + 1], 1]])
        assert np.array_equal(res.points[res.offsets[s]:res.offsets[s + 1]], ep[ids])
    want = compute_eval_data_from_hair_gs(mixed, compute_edges=True)
    got = strand_eval_data(res)
    for name in ("points", "directions", "points_id_to_strand_id"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert np.array_equal(got.edges, want.edges)
    path = tmp_path / "hair_eval_data.npz"
    write_strands_npz(str(path), res)
    assert sorted(np.load(path).files) == ["directions", "edges", "points", "points_id_to_strand_id"]
    back = load_hair_eval_data_npz(str(path))
    assert back.points.tobytes() == want.points.tobytes() and np.array_equal(back.points_id_to_strand_id, want.points_id_to_strand_id)
    assert np.array_equal(back.edges, want.edges)


def test_npz_leaves_out_segments_without_a_direction(collapsed, tmp_path):
    from data.eval_data import load_hair_eval_data_npz
    from data.strand_files import strand_eval_data, write_strands_npz
    from scene.strand_export import resample_strands
    m, has = collapsed
    res = resample_strands(m, points=0)
    d = strand_eval_data(res)
    offsets, rows, _, ep, _ = R.strand_tables(m)
    live = np.any(ep[rows[:, 1]] != ep[rows[:, 0]], axis=1)
    assert 0 < live.sum() < live.shape[0] and d.points.shape[0] == live.sum()
    assert np.array_equal(d.points, ep[rows[live, 0]]) and np.all(np.isfinite(d.directions))
    assert np.allclose(np.linalg.norm(d.directions, axis=1), 1, atol=1e-6)
    assert 2 not in d.points_id_to_strand_id                              # the strand that is one point has no oriented point
    sid = d.points_id_to_strand_id
    assert np.array_equal(d.edges[:, 1], d.edges[:, 0] + 1) and np.all(sid[d.edges[:, 0]] == sid[d.edges[:, 1]])
    assert d.edges.shape[0] == live.sum() - np.unique(sid).shape[0]       # a chain per strand
    write_strands_npz(str(tmp_path / "c.npz"), res)
    assert np.all(np.isfinite(load_hair_eval_data_npz(str(tmp_path / "c.npz")).directions))


def _hand_model():
    """Four straight strands along x: 1, 2, 3 and 5 segments of 1 mm, 2 mm, 0.5 mm and 1 mm; rooted at y = 0, 1, 2, 3 cm."""
    lines = []
    for k, (n, step) in enumerate(((1, 1e-3), (2, 2e-3), (3, 5e-4), (5, 1e-3))):
        lines.append(np.stack([np.arange(n + 1) * step, np.full(n + 1, 0.01 * k), np.zeros(n + 1)], axis=1).astype(np.float32))
    return R.model_from_polylines(lines, seed=1)


def test_filters_on_a_hand_built_model():
    from scene.strand_export import resample_strands
    m = _hand_model()
    ids = lambda **kw: resample_strands(m, points=4, **kw).strand_ids.tolist()
    assert ids() == [0, 1, 2, 3]
    assert ids(min_segments=2) == [1, 2, 3] and ids(min_segments=4) == [3] and ids(min_segments=6) == []
    assert ids(min_length=0.0012) == [1, 2, 3] and ids(min_length=0.003) == [1, 3] and ids(min_length=0.003, min_segments=3) == [3]
    res = resample_strands(m, points=4, min_length=0.003)
    assert np.array_equal(res.offsets, [0, 4, 8]) and np.allclose(res.length, [0.004, 0.005], rtol=1e-6)
    assert np.array_equal(res.points, R.reference_export(m, 4, kept=[1, 3])[0])
    # roots of strands 1 and 2 moved 3 mm and 7 mm away from their strands
    roots = np.asarray(m.ref_strand_root, np.float64).copy()
    roots[1, 2] += 0.003
    roots[2, 2] += 0.007
    m.ref_strand_root = roots
    assert ids(max_root_distance=0.005) == [0, 1, 3] and ids(max_root_distance=0.001) == [0, 3]
    assert ids(max_root_distance=0.005, min_segments=2) == [1, 3]
    assert resample_strands(m, points=0, max_root_distance=0.001).offsets.tolist() == [0, 2, 8]
    m.ref_strand_root = np.empty(0)
    with pytest.raises(ValueError, match="root"):
        resample_strands(m, points=4, max_root_distance=0.005)
    with pytest.raises(ValueError, match="points"):
        resample_strands(m, points=1)


def test_hair_and_data_files_round_trip(mixed, tmp_path):
    from data.cy_hair import read_cy_hair
    from data.strand_files import read_usc_hair, write_strands_cy, write_strands_usc
    from scene.strand_export import StrandExport, resample_strands
    for M in (0, 7):
        res = resample_strands(mixed, points=M, min_segments=2)
        write_strands_cy(str(tmp_path / "a.hair"), res)
        hf = read_cy_hair(str(tmp_path / "a.hair"))
        cnt = res.offsets[1:] - res.offsets[:-1]
        assert hf.header.hair_count == res.n_strands and hf.header.point_count == res.points.shape[0] and hf.header.arrays == 31
        assert np.array_equal(hf.segments, cnt - 1) and hf.segments.dtype == np.uint16
        assert np.array_equal(hf.points, res.points) and np.array_equal(hf.thickness, res.attrs[:, 4])
        assert np.array_equal(hf.transparency, np.float32(1) - res.attrs[:, 3]) and np.array_equal(hf.colors, res.attrs[:, :3])
        write_strands_usc(str(tmp_path / "a.data"), res)
        pts, off = read_usc_hair(str(tmp_path / "a.data"))
        assert np.array_equal(pts, res.points) and np.array_equal(off, res.offsets) and pts.dtype == np.float32
        raw = open(tmp_path / "a.data", "rb").read()
        assert struct.unpack_from("<ii", raw, 0) == (res.n_strands, int(cnt[0])) and len(raw) == 4 + 4 * res.n_strands + 12 * pts.shape[0]
    long = StrandExport(np.zeros((65537 + 1, 3), np.float32), np.zeros((65537 + 1, 5), np.float32), np.array([0, 65538]), np.array([0]),
                        np.zeros(1))
    with pytest.raises(ValueError, match="65535"):
        write_strands_cy(str(tmp_path / "b.hair"), long)


def test_write_cy_hair_keeps_its_bytes_without_the_new_keywords(tmp_path):
    from data.cy_hair import HEADER, read_cy_hair, write_cy_hair
    pts = np.arange(18, dtype=np.float32).reshape(6, 3)
    col = np.linspace(0, 1, 18, dtype=np.float32).reshape(6, 3)
    write_cy_hair(str(tmp_path / "a.hair"), pts, segments=[1, 3], colors=col, info="x")
    want = HEADER.pack(b"HAIR", 2, 6, 1 | 2 | 16, 0, 1.0, 0.0, 1.0, 1.0, 1.0, b"x") + np.array([1, 3], "<u2").tobytes() + pts.tobytes() + col.tobytes()
    assert open(tmp_path / "a.hair", "rb").read() == want
    write_cy_hair(str(tmp_path / "b.hair"), pts, d_segments=2)
    assert open(tmp_path / "b.hair", "rb").read() == HEADER.pack(b"HAIR", 2, 6, 2, 2, 1.0, 0.0, 1.0, 1.0, 1.0, b"") + pts.tobytes()
    th, tr = np.arange(6, dtype=np.float32), np.arange(6, dtype=np.float32) / 8
    write_cy_hair(str(tmp_path / "c.hair"), pts, segments=[1, 3], colors=col, thickness=th, transparency=tr)
    hf = read_cy_hair(str(tmp_path / "c.hair"))
    assert hf.header.arrays == 31 and np.array_equal(hf.thickness, th) and np.array_equal(hf.transparency, tr) and np.array_equal(hf.colors, col)


def test_ply_layouts_round_trip(mixed, tmp_path):
    from data.hair_data import hsv2rgb_u8
    from data.strand_files import strand_colours, strand_edges, write_strands_ply
    from scene.strand_export import resample_strands
    from utils.ply import read_ply
    res = resample_strands(mixed, points=5)
    N, K = res.points.shape[0], res.n_strands
    edges = strand_edges(res)
    assert edges.shape == (K * 4, 2) and np.array_equal(edges[:5], [[0, 1], [1, 2], [2, 3], [3, 4], [5, 6]])
    write_strands_ply(str(tmp_path / "e.ply"), res, faces=False, colour="model")
    raw = open(tmp_path / "e.ply", "rb").read()
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {N}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement edge {K * 4}\nproperty int vertex1\n"
              "property int vertex2\nend_header\n").encode()
    assert raw.startswith(header) and len(raw) == len(header) + 15 * N + 8 * K * 4
    (vn, v), (en, e) = read_ply(str(tmp_path / "e.ply"))
    assert (vn, en) == ("vertex", "edge")
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), res.points)
    rgb = np.stack([v["red"], v["green"], v["blue"]], 1)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, np.rint(res.attrs[:, :3] * np.float32(255)).astype(np.uint8))
    assert np.array_equal(np.stack([e["vertex1"], e["vertex2"]], 1), edges)
    write_strands_ply(str(tmp_path / "f.ply"), res, faces=True, colour="strand")
    raw = open(tmp_path / "f.ply", "rb").read()
    E = K * 4
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {N + E}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {E}\n"
              "property list uchar int vertex_indices\nend_header\n").encode()
    assert raw.startswith(header) and len(raw) == len(header) + 15 * (N + E) + 13 * E
    (vn, v), (fn, f) = read_ply(str(tmp_path / "f.ply"))
    assert (vn, fn) == ("vertex", "face") and f["vertex_indices"].shape == (E, 3) and f["vertex_indices"].dtype == np.int32
    assert np.array_equal(f["vertex_indices"], np.column_stack([edges[:, 0], N + np.arange(E), edges[:, 1]]))
    xyz = np.stack([v["x"], v["y"], v["z"]], 1)
    assert np.array_equal(xyz[:N], res.points)
    assert np.array_equal(xyz[N:], ((res.points[edges[:, 0]] + res.points[edges[:, 1]]) / 2).astype(np.float32))
    rgb = np.stack([v["red"], v["green"], v["blue"]], 1)
    hues = np.linspace(0, 180, K).astype(np.uint8)
    assert np.array_equal(rgb[:N], np.repeat(np.stack([hsv2rgb_u8(h) for h in hues]), 5, axis=0))
    assert np.array_equal(rgb[:N], strand_colours(res, "strand"))
    assert np.array_equal(rgb[N:], ((rgb[edges[:, 0]].astype(np.float64) + rgb[edges[:, 1]]) / 2).astype(np.uint8))


def test_ply_lists_and_scalar_bytes(tmp_path):
    from utils.ply import read_ply, write_ply
    v = np.zeros(2, dtype=[("x", "<f4"), ("red", "u1"), ("k", "<i4")])
    v["x"], v["red"], v["k"] = [1.5, -2.0], [7, 255], [3, -4]
    write_ply(str(tmp_path / "s.ply"), [("vertex", v)])
    # a scalar-only file keeps the bytes it has always had
    want = b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty uchar red\nproperty int k\nend_header\n" \
        + struct.pack("<fBi", 1.5, 7, 3) + struct.pack("<fBi", -2.0, 255, -4)
    assert open(tmp_path / "s.ply", "rb").read() == want
    f = np.zeros(3, dtype=[("q", "<f4"), ("vertex_indices", "<i4", (3,)), ("w", "<u2", (2,))])
    f["q"], f["vertex_indices"], f["w"] = [0.5, 1.5, 2.5], np.arange(9).reshape(3, 3), [[1, 2], [3, 4], [5, 6]]
    write_ply(str(tmp_path / "l.ply"), [("vertex", v), ("face", f)])
    raw = open(tmp_path / "l.ply", "rb").read()
    assert b"property float q\nproperty list uchar int vertex_indices\nproperty list uchar ushort w\nend_header\n" in raw
    assert raw.endswith(struct.pack("<fB3iB2H", 2.5, 3, 6, 7, 8, 2, 5, 6))
    els = read_ply(str(tmp_path / "l.ply"))
    assert els[0][1].tobytes() == v.tobytes() and els[1][1].dtype == f.dtype and els[1][1].tobytes() == f.tobytes()
    # ASCII and big-endian files with the same content
    head = raw[:raw.index(b"end_header")]
    rows_v = "".join(f"{a} {b} {c}\n" for a, b, c in v.tolist())
    rows_f = "".join(f"{q} 3 {i[0]} {i[1]} {i[2]} 2 {w[0]} {w[1]}\n" for q, i, w in f.tolist())
    open(tmp_path / "a.ply", "wb").write(head.replace(b"binary_little_endian", b"ascii") + b"end_header\n" + (rows_v + rows_f).encode())
    els = read_ply(str(tmp_path / "a.ply"))
    assert els[0][1].tobytes() == v.tobytes() and els[1][1].tobytes() == f.tobytes()
    big = b"".join(struct.pack(">fBi", *r) for r in v.tolist()) + b"".join(struct.pack(">fB3iB2H", q, 3, *i, 2, *w) for q, i, w in f.tolist())
    open(tmp_path / "b.ply", "wb").write(head.replace(b"binary_little_endian", b"binary_big_endian") + b"end_header\n" + big)
    els = read_ply(str(tmp_path / "b.ply"))
    assert els[0][1].tobytes() == v.tobytes() and els[1][1].tobytes() == f.tobytes()
    # ragged lists are still refused, in both encodings
    ragged = b"".join(struct.pack("<fBi", *r) for r in v.tolist()) + struct.pack("<fB3iB2H", 0.5, 3, 0, 1, 2, 2, 1, 2) \
        + struct.pack("<fB4iB2H", 1.5, 4, 3, 4, 5, 6, 2, 3, 4) + struct.pack("<fB3iB2H", 2.5, 3, 6, 7, 8, 2, 5, 6)
    open(tmp_path / "r.ply", "wb").write(head + b"end_header\n" + ragged)
    with pytest.raises(ValueError, match="different lengths"):
        read_ply(str(tmp_path / "r.ply"))
    open(tmp_path / "ra.ply", "wb").write(head.replace(b"binary_little_endian", b"ascii") + b"end_header\n"
                                          + (rows_v + rows_f.replace("3 3 4 5", "4 3 4 5 9")).encode())
    with pytest.raises(ValueError, match="different lengths"):
        read_ply(str(tmp_path / "ra.ply"))
    with pytest.raises(TypeError):
        write_ply(str(tmp_path / "x.ply"), [("face", np.zeros(1, dtype=[("m", "<f4", (2, 2))]))])


def test_driver_writes_every_format_and_refuses_a_cloud(mixed, tmp_path, capsys):
    import export_strands
    from data.cy_hair import read_cy_hair
    from data.eval_data import load_hair_eval_data_npz
    from data.strand_files import read_usc_hair
    from scene.strand_export import resample_strands
    from utils.ply import read_ply, write_ply
    model = tmp_path / "out"
    os.makedirs(model / "point_cloud" / "iteration_3")
    os.makedirs(model / "point_cloud" / "iteration_12")
    mixed.save_ply(str(model / "point_cloud" / "iteration_12" / "point_cloud.ply"))
    out = tmp_path / "export" / "strands"
    argv = ["-m", str(model), "-o", str(out), "--device", "cpu", "--points", "9", "--min_segments", "2"]
    for f in export_strands.FORMATS:
        argv += ["--format", f]
    res, paths = export_strands.main(argv)
    text = capsys.readouterr().out
    assert "iteration_12" in text and "Strands: 10, kept: 8, points: 72" in text
    assert {k: os.path.basename(p) for k, p in paths.items()} == {"hair": "strands.hair", "usc": "strands.data", "ply_edges": "strands.ply",
                                                                   "ply_faces": "strands_faces.ply", "npz": "strands.npz"}
    want = resample_strands(mixed, points=9, min_segments=2)
    assert np.array_equal(res.points, want.points) and np.array_equal(res.attrs, want.attrs) and np.array_equal(res.strand_ids, want.strand_ids)
    hf = read_cy_hair(paths["hair"])
    assert hf.header.hair_count == 8 and np.array_equal(hf.points, want.points) and np.all(hf.segments == 8)
    assert np.array_equal(read_usc_hair(paths["usc"])[0], want.points)
    assert read_ply(paths["ply_edges"])[1][1].shape[0] == 8 * 8 and read_ply(paths["ply_faces"])[1][1]["vertex_indices"].shape == (64, 3)
    ev = load_hair_eval_data_npz(paths["npz"])
    assert ev.points.shape == (64, 3) and set(ev.points_id_to_strand_id.tolist()) == set(want.strand_ids.tolist())
    # a strand PLY named directly, the joints, the default format
    res0, paths0 = export_strands.main(["-m", str(model / "point_cloud" / "iteration_12" / "point_cloud.ply"), "-o", str(tmp_path / "j.hair"),
                                        "--device", "cpu", "--points", "0"])
    assert list(paths0) == ["hair"] and paths0["hair"] == str(tmp_path / "j.hair")
    assert read_cy_hair(paths0["hair"]).header.point_count == mixed.endpoint_pairs.shape[0] + 10
    cloud = tmp_path / "cloud.ply"
    write_ply(str(cloud), [("vertex", np.zeros(3, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("opacity", "<f4")]))])
    with pytest.raises(ValueError, match="cloud"):
        export_strands.main(["-m", str(cloud), "-o", str(tmp_path / "c"), "--device", "cpu"])
