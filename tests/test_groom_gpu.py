"""The groom interpolation on the GPU (csrc/hgs_groom.hip through scene/groom.py): the device path against the loop restatement of
the contract (tests/groom_reference.py) bit for bit on the size grid and the hard inputs of tests/groom_cases.py, a second launch, a
side stream, the numpy path, and the driver in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import groom_cases as GC
from tests import groom_reference as GR
from tests.test_groom_cpu import _cos_max, assert_search_equal, driver_model, reference_blend

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _up(*arrays):
    return tuple(torch.as_tensor(a, device="cuda") for a in arrays)


def _search(gp_d, roots_d, k, max_d2, cos_max):
    from scene.groom import search_device
    return tuple(t.cpu().numpy() for t in search_device(gp_d, roots_d, k, max_d2, cos_max))


def _guides(gp, ga):
    from scene.strand_export import StrandExport
    K, M, C = ga.shape
    return StrandExport(gp.reshape(-1, 3), ga.reshape(-1, C), np.arange(K + 1, dtype=np.int64) * M, np.arange(K, dtype=np.int64), np.zeros(K))


@pytest.mark.parametrize("K", GC.KS)
def test_device_search_matches_the_loop_restatement(K):
    gp, _, roots = GC.grid_case(K)
    cands, ch = GR.grid_candidates(K)
    gp_d, roots_d = _up(gp, roots)
    for k in GC.KNN:
        for max_d2 in GC.MAX_D2:
            for angle in GC.ANGLES:
                ref = GR.search(cands, ch, k, max_d2, _cos_max(angle))
                for N in GC.NS:
                    got = _search(gp_d, roots_d[:N], k, max_d2, _cos_max(angle))
                    assert_search_equal(got, tuple(a[:N] for a in ref), f"K={K} k={k} max_d2={max_d2} angle={angle} N={N}")


def test_every_k_has_its_kernel():
    """k = 1..8 are eight instantiations: each against the restatement at the tile edge."""
    gp, _, roots = GC.grid_case(257)
    cands, ch = GR.grid_candidates(257)
    gp_d, roots_d = _up(gp, roots)
    for k in range(1, 9):
        assert_search_equal(_search(gp_d, roots_d, k, 4.0, _cos_max(60.0)), GR.search(cands, ch, k, 4.0, _cos_max(60.0)), f"k={k}")


@pytest.mark.parametrize("case", GC.hard_cases(), ids=lambda c: c[0])
def test_hard_inputs_on_the_device(case):
    from scene.groom import blend_device
    name, gp, ga, roots, k, max_d2, angle, expect = case
    cos_max = _cos_max(angle)
    ref = GR.search(GR.candidates(gp, roots), GR.chords(gp), k, max_d2, cos_max)
    gp_d, ga_d, roots_d = _up(gp, ga, roots)
    got = _search(gp_d, roots_d, k, max_d2, cos_max)
    assert_search_equal(got, ref, name)
    if expect is not None:
        assert [[int(g) for g in row if g >= 0] for row in got[0]] == expect
    kept = np.nonzero(got[3] > 0)[0]
    idx_d, w_d, kept_d = _up(got[0], got[2], kept.astype(np.int32))
    pts, att = (t.cpu().numpy() for t in blend_device(gp_d, ga_d, roots_d, idx_d, w_d, kept_d))
    rp, ra, rk = GR.blend(gp, ga, roots, ref[0], ref[2], ref[3])
    assert np.array_equal(kept, rk) and GR.same_bytes(pts, rp) and GR.same_bytes(att, ra), name


def _device(case, stream=None):
    from scene.groom import interpolate_strands
    N, K, k, M, C, max_d2, angle = case
    gp, ga, roots = GC.grid_case(K, M, C)
    kw = dict(k=k, max_guide_distance=None if np.isinf(max_d2) else float(np.sqrt(max_d2)), max_angle=angle, first_id=1000)
    if stream is None:
        return interpolate_strands(_guides(gp, ga), roots[:N], device="cuda", **kw)
    with torch.cuda.stream(stream):
        res = interpolate_strands(_guides(gp, ga), roots[:N], device="cuda", **kw)
    stream.synchronize()
    return res


def _same(a, b):
    return (all(GR.same_bytes(np.asarray(x), np.asarray(y)) for x, y in zip(a.strands, b.strands)) and GR.same_bytes(a.root_ids, b.root_ids)
            and a.n_dropped == b.n_dropped and GR.same_bytes(a.n_guides, b.n_guides))


@pytest.mark.parametrize("case", GC.BLEND_CASES, ids=lambda c: "N{}-K{}-k{}-M{}-C{}".format(*c[:5]))
def test_device_path_matches_the_loop_restatement(case):
    N, K, k, M, C, max_d2, angle = case
    res = _device(case)
    s, pts, att, kept, length = reference_blend(case)
    assert np.array_equal(res.root_ids, kept) and res.n_dropped == N - kept.shape[0]
    assert GR.same_bytes(res.strands.points, pts) and GR.same_bytes(res.strands.attrs, att)
    assert GR.same_bytes(res.strands.length, length) and GR.same_bytes(res.n_guides, s[3][kept])
    assert np.array_equal(res.strands.offsets, np.arange(kept.shape[0] + 1) * M) and np.array_equal(res.strands.strand_ids, 1000 + kept)
    # a second launch, and the same call on a side stream, give the same bytes
    assert _same(_device(case), res)
    assert _same(_device(case, torch.cuda.Stream()), res)


def test_device_path_matches_the_numpy_path():
    """One mixed case with dropped roots: the two product paths against each other."""
    from scene.groom import interpolate_strands
    gp, ga, roots = GC.grid_case(513, 65, 5)
    guides = _guides(gp, ga)
    kw = dict(k=8, max_guide_distance=1.0, max_angle=60.0)
    dev, host = interpolate_strands(guides, roots, device="cuda", **kw), interpolate_strands(guides, roots, **kw)
    assert 0 < host.n_dropped < 257 and host.n_guides.min() == 1 and host.n_guides.max() > 4
    assert _same(dev, host)
    with pytest.raises(ValueError, match="native mode"):
        interpolate_strands(guides._replace(offsets=np.concatenate([[0, 1], guides.offsets[2:]])), roots, device="cuda")


def test_device_wrappers_check_their_tensors():
    import hgs_runtime as rt
    from scene.groom import blend_device, search_device
    gp, ga, roots = GC.grid_case(7, 3, 2)
    gp_d, ga_d, roots_d = _up(gp, ga, roots)
    with pytest.raises(rt.HgsError):
        search_device(torch.as_tensor(gp), roots_d, 4, np.inf, 0.5)            # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError, match="k = 9"):
        search_device(gp_d, roots_d, 9, np.inf, 0.5)
    idx, _, w, count = search_device(gp_d, roots_d, 4, np.inf, 0.5)
    kept = torch.nonzero(count > 0).reshape(-1).to(torch.int32)
    blend_device(gp_d, ga_d, roots_d, idx, w, kept)
    bad = kept.clone()
    bad[-1] = 257
    with pytest.raises(rt.HgsError, match="out of range"):
        blend_device(gp_d, ga_d, roots_d, idx, w, bad)
    with pytest.raises(rt.HgsError):
        blend_device(gp_d, ga_d, roots_d, idx, w, kept.to(torch.int64))
    with pytest.raises(rt.HgsError):
        blend_device(gp_d, ga_d, roots_d[:100], idx, w, kept)


def test_driver_on_the_device_in_a_child_process(tmp_path):
    """export_strands.py --interpolate --device cuda as a process of its own writes the bytes the --device cpu run writes: guides
    first, then the interpolated strands."""
    import export_strands
    model, n_roots = driver_model(tmp_path)
    common = ["-m", str(model), "--format", "hair", "--format", "usc", "--points", "20", "--interpolate", "--guides", "3", "--max_guide_distance", "0.5"]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "hair-gs_amd", "export_strands.py")] + common + ["-o", str(tmp_path / "dev"), "--device", "cuda"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"Interpolated: {n_roots} roots, 1 dropped" in run.stdout
    export_strands.main(common + ["-o", str(tmp_path / "host"), "--device", "cpu"])
    for ext in (".hair", ".data"):
        d, h = open(tmp_path / ("dev" + ext), "rb").read(), open(tmp_path / ("host" + ext), "rb").read()
        assert len(d) == len(h) and d == h, ext
