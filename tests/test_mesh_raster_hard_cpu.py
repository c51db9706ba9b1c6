"""The rasterizer of the dataset synthesis on the hard cases of tests/mesh_raster_cases.py, without a GPU: the numpy path of
scene/mesh_renderer.py against the brute force of tests/mesh_raster_reference.py (image bytes, gray bytes, dropped count), the
snapped coordinates each case intends, and, for every switch of the reference, the cases on which getting that decision wrong
changes the picture: the evidence that the cases reach it."""
import numpy as np
import pytest

from tests.mesh_raster_cases import CASES, COVERED_ONCE, I4
from tests.mesh_raster_cases import expected as ref_of
from tests.mesh_raster_reference import INT_MIN, SWITCHES, reference


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_path_equals_reference(name):
    from scene.mesh_renderer import render_views
    models, views, projs, W, H, light, bg, sel = CASES[name]()
    img, dropped, gray = render_views(models, views, projs, W, H, light, mesh_indices=sel, background=bg, return_gray=True)
    ref = ref_of(name)
    assert img.shape == ref.rgb.shape and dropped == ref.dropped
    bad = (img != ref.rgb).any(-1)
    assert not bad.any(), f"{name}: {int(bad.sum())} pixel(s) differ, first (view, image row, column) {np.argwhere(bad)[0].tolist()}"
    assert np.array_equal(gray, ref.gray)


@pytest.mark.parametrize("name", list(CASES))
def test_intended_snapped_coordinates(name):
    models, views, projs, W, H, light, bg, sel = CASES[name]()
    chosen = sorted(set(sel)) if sel is not None else range(len(models))
    if not all(hasattr(models[i], "intent") for i in chosen):
        assert name in ("dropped_rules", "shading_persp")            # placed in world space under a camera
        return
    want = np.concatenate([models[i].intent for i in chosen]).reshape(-1, 2)
    ref = ref_of(name)
    if np.array_equal(np.asarray(views), I4) and np.array_equal(np.asarray(projs), I4):
        z, w, X, Y = ref.vertices[0]
        assert (X != INT_MIN).all() and np.array_equal(X, want[:, 0]) and np.array_equal(Y, want[:, 1])
        assert (w == 1.0).all()
    else:
        assert name == "views_3" and ref.V == 3                      # (its models are those of identity cases, checked there)


def test_shared_edges_cover_each_centre_once():
    for name, pixels in COVERED_ONCE.items():
        cov = ref_of(name).coverage[0]
        assert cov.max() == 1
        assert all(cov[j, i] == 1 for i, j in pixels)


def test_cases_reach_what_they_claim():
    """Properties of the cases that no comparison would miss silently: drops, discards, culls, list lengths and frame sizes."""
    r = ref_of("dropped_rules")
    assert r.dropped_per_view[0] > 0 and r.dropped_per_view[1] > 0 and r.dropped_per_view[0] != r.dropped_per_view[1]
    gone = [r.vertices[v][2] == INT_MIN for v in range(2)]
    assert gone[0].sum() not in (0, r.NV) and not np.array_equal(gone[0], gone[1])
    assert np.isinf(r.vertices[0][0]).any() and (r.vertices[0][1] == 0.0).any()          # c.w == 0
    assert max(len(s) for s in ref_of("hot_tile_300").tiles[0]) > 256
    assert max(len(s) for s in ref_of("hot_tile_1100").tiles[0]) > 1024
    assert [ref_of(f"prims_{n}").n_prims for n in (255, 256, 257)] == [255, 256, 257]
    assert ref_of("all_empty").n_prims == 0 and ref_of("models_64").n_prims > 64
    w = ref_of("size_16384x2")
    assert w.TX == 512 and max(int(np.abs(v[2]).max()) for v in w.vertices) == 1 << 22
    assert all(len(s) > 0 for s in ref_of("tris_hard").tiles[0])                             # the large triangle reaches every tile
    holds = lambda name, draw: {t for t, s in enumerate(ref_of(name).tiles[0]) if draw in s}
    assert holds("lines_directions", 4) == {0, 4, 8}              # a diagonal's tiles, not the 9 of its bounding box
    assert holds("lines_tile_edges", 19) == {0, 3}                # the band straddles y = 32 inside tile column 0
    far = ref_of("lines_far")
    assert int(np.abs(far.vertices[0][2]).max()) == 1 << 22 and (np.abs(far.vertices[0][2]) == 4194278).any()
    sh = ref_of("shading_persp").vertices[0][1]
    assert sh.max() / sh.min() > 9.9
    for name in CASES:                                                                       # no case is an empty picture
        r = ref_of(name)
        assert (r.coverage.reshape(r.V, -1).max(1) > 0).all() == (name != "all_empty"), name


@pytest.mark.parametrize("switch", SWITCHES)
def test_every_switch_is_caught(switch):
    """Each decision the reference can get wrong on purpose changes the bytes of at least one named case."""
    expect = {"closed_interval": "lines_directions", "strict_xmajor": "lines_directions", "trunc_division": "lines_wide",
              "half_width_up": "lines_tile_edges", "mirrored_top_left": "tris_shared_edges", "last_draw_wins": "depth_ties",
              "keep_far": "depth_ties", "affine": "shading_persp"}[switch]
    small = [n for n in CASES if not n.startswith(("size_16384", "hot_tile_1100"))]
    caught = []
    for name in [expect] + [n for n in small if n != expect]:
        models, views, projs, W, H, light, bg, sel = CASES[name]()
        got = reference(models, views, projs, W, H, light, bg, sel, **{switch: True})
        ref = ref_of(name)
        n = int((got.rgb != ref.rgb).any(-1).sum())
        if n or got.tiles != ref.tiles:
            caught.append(f"{name} ({n} px)")
        if len(caught) >= 3 and name != expect:
            break
    print(f"switch {switch}: caught by {', '.join(caught)}")
    assert caught and caught[0].startswith(expect + " ("), f"{switch}: expected {expect} to catch it, got {caught}"
    assert not caught[0].endswith("(0 px)")
