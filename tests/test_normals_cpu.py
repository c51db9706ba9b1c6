"""Point-cloud normals without a GPU: the host path is unchanged and stays the default of every new keyword, the device path's
argument checks raise before the native library is touched, the driver refuses --normals device on the CPU, and the scratch
size of the C entry is well-behaved."""
import inspect
import os

import numpy as np
import pytest

from tests import normals_fixtures as F


def test_host_path_is_what_it_was():
    from utils.normals import estimate_pointcloud_normals
    p = F.cloud("cloud")[:5000]
    want = F.host_restatement(p, 50)
    assert np.array_equal(estimate_pointcloud_normals(p), want)
    assert np.array_equal(estimate_pointcloud_normals(p, device=None), want)
    assert np.array_equal(estimate_pointcloud_normals(p, 50, 1 << 10, "cpu"), want)       # (chunking does not change a row)
    assert estimate_pointcloud_normals(np.zeros((0, 3))).shape == (0, 3)


def test_new_keywords_default_to_the_host_path():
    import synthesize
    from data import hair_data, head_data
    from utils import normals
    assert inspect.signature(normals.estimate_pointcloud_normals).parameters["device"].default is None
    for fn in (hair_data.load_hair_from_usc_dataset, head_data.load_head_from_usc_dataset, head_data.load_head_from_cy_dataset):
        assert inspect.signature(fn).parameters["normals_device"].default is None
    assert normals.DEVICE_MAX_NEIGHBORS == 64
    assert "--normals" in synthesize.__doc__


def test_device_argument_checks_need_no_library(monkeypatch):
    import hgs_runtime as rt
    import torch
    from utils.normals import estimate_pointcloud_normals, estimate_pointcloud_normals_device

    def touched():
        raise AssertionError("the native library was touched before the arguments were checked")
    monkeypatch.setattr(rt, "lib", touched)
    p = F.cloud("cloud")[:200]
    with pytest.raises(ValueError, match="64"):
        estimate_pointcloud_normals(p, 65, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        estimate_pointcloud_normals(p[:, :2], device="cuda")
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            estimate_pointcloud_normals(q, device="cuda")
    assert estimate_pointcloud_normals(np.zeros((0, 3)), device="cuda").shape == (0, 3)
    with pytest.raises(ValueError, match="64"):
        estimate_pointcloud_normals_device(torch.from_numpy(p), 65)
    with pytest.raises(ValueError, match="shape"):
        estimate_pointcloud_normals_device(torch.from_numpy(p[:, :2].copy()))
    with pytest.raises(TypeError):
        estimate_pointcloud_normals_device(torch.from_numpy(p))            # a CPU tensor
    with pytest.raises(TypeError):
        estimate_pointcloud_normals_device(p)                              # not a tensor
    # K clamps to N before the limit applies: 65 neighbours of 60 points are 60
    with pytest.raises(TypeError):
        estimate_pointcloud_normals_device(torch.from_numpy(p[:60]), 65)


def _scene_files(tmp_path):
    from tests.synth_fixtures import sphere_mesh, write_obj, write_usc
    hair, head = tmp_path / "strands.data", tmp_path / "head.obj"
    write_usc(str(hair), n_long=100, seed=3)
    v, f, n = sphere_mesh()
    write_obj(str(head), v, f, n)
    return ["--dataset", "usc_hair_salon", "--hair", str(hair), "--head", str(head), "--pct_strands", "1", "--cameras", "2",
            "--height", "64", "--width", "64", "--cam_z", "0.45", "--device", "cpu"]


def test_driver_flag(tmp_path, capsys):
    import synthesize
    common = _scene_files(tmp_path)
    with pytest.raises(SystemExit) as e:
        synthesize.main(common + ["-o", str(tmp_path / "bad"), "--normals", "device"])
    assert e.value.code == 2 and "--normals device" in capsys.readouterr().err
    assert not (tmp_path / "bad").exists()
    synthesize.main(common + ["-o", str(tmp_path / "plain")])
    assert "normals: host" in capsys.readouterr().out
    synthesize.main(common + ["-o", str(tmp_path / "host"), "--normals", "host"])
    files = sorted(os.path.relpath(os.path.join(d, n), tmp_path / "plain") for d, _, ns in os.walk(tmp_path / "plain") for n in ns)
    assert len(files) >= 2 * 4 + 5
    assert files == sorted(os.path.relpath(os.path.join(d, n), tmp_path / "host") for d, _, ns in os.walk(tmp_path / "host") for n in ns)
    for n in files:
        assert (tmp_path / "plain" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n


def test_scratch_size():
    import hgs_runtime as rt
    L = rt.lib()
    sizes = [int(L.hgs_pointcloud_normals_scratch_bytes(n, 50)) for n in (0, 1, 7, 64, 4096, 4097, 50000, 200000, 1000000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert int(L.hgs_pointcloud_normals_scratch_bytes(-5, 50)) == sizes[0]
    for k in (1, 3, 64):
        assert int(L.hgs_pointcloud_normals_scratch_bytes(1000000, k)) % 256 == 0
    # the sorted positions and the keys alone: 32 + 8 bytes per point
    assert sizes[-1] >= 40 * 1000000
