"""The head push-out on the GPU (csrc/hgs_collide.hip through scene/strand_collide.py): the kernel against the numpy path and the loop
restatement of the contract (tests/collide_reference.py) bit for bit on the hard cases and strand counts of tests/collide_cases.py and
on the analytic head, a second launch and a side stream, the wrapper's checks, the C entry point's refusals on device buffers, and the
driver in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import collide_cases as CC
from tests import collide_reference as CR
from tests.test_collide_cpu import assert_same, counted_reference, driver_scene, reference, sphere_result

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _device(pts, off, sdf, margin, skin, iters, stream=None):
    from scene.strand_collide import resolve_device
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    if stream is None:
        res = resolve_device(pts_d, off_d, sdf, margin, skin, iters)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            res = resolve_device(pts_d, off_d, sdf, margin, skin, iters)
        stream.synchronize()
    return tuple(t.cpu().numpy() for t in res)


@pytest.mark.parametrize("name", CC.HARD_NAMES)
def test_kernel_matches_the_numpy_path_and_the_restatement(name):
    from scene.strand_collide import resolve_numpy
    pts, off, fname, margin, skin, iters = CC.hard_cases()[name]
    sdf = CC.field(fname)
    got = _device(pts, off, sdf, margin, skin, iters)
    assert_same(got, resolve_numpy(pts, off, sdf, margin, skin, iters), name + " (numpy)")
    assert_same(got, reference(name)[:3], name + " (loop)")


@pytest.mark.parametrize("K", CC.KS)
def test_kernel_at_every_strand_count(K):
    fname, margin, skin, iters = CC.COUNTED
    pts, off = CC.first_strands(*CC.counted_strands(), K)
    ref = counted_reference()
    got = _device(pts, off, CC.field(fname), margin, skin, iters)
    assert_same(got, (ref[0][:off[K]], ref[1][:K], ref[2][:K]), f"K={K}")


@pytest.mark.parametrize("grid", CC.SPHERE_GRIDS)
def test_kernel_on_the_analytic_head(grid):
    pts, off = CC.sphere_scene()
    for margin in CC.SPHERE_MARGINS:
        for iters in CC.SPHERE_ITERS:
            got = _device(pts, off, CC.field(f"sphere{grid}"), margin, None, iters)
            assert_same(got, sphere_result(grid, margin, iters), f"grid={grid} margin={margin} iters={iters}")
            assert int(got[2].sum()) == 0 and int(got[1].sum()) > 0


def test_two_runs_and_a_side_stream_give_equal_bytes():
    pts, off, fname, margin, skin, iters = CC.hard_cases()["ragged_fine_grid_i32"]
    sdf = CC.field(fname)
    first = _device(pts, off, sdf, margin, skin, iters)
    assert_same(_device(pts, off, sdf, margin, skin, iters), first, "second run")
    assert_same(_device(pts, off, sdf, margin, skin, iters, torch.cuda.Stream()), first, "side stream")
    assert first[1].sum() > 0


def test_resolve_head_on_the_device_equals_the_numpy_path():
    """The product's entry point on both devices: points, lengths and every figure of the report."""
    from scene.strand_collide import resolve_head
    from scene.strand_export import StrandExport
    for (pts, off), fname, margin in ((CC.sphere_scene(), "sphere32", 0.02), (CC.special_strands(), "sphere9", 0.05), (CC.ragged_strands(), "sphere24", 0.0)):
        K = off.shape[0] - 1
        strands = StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), off, np.arange(K, dtype=np.int64), np.zeros(K))
        host, hs = resolve_head(strands, CC.field(fname), margin=margin)
        dev, ds = resolve_head(strands, CC.field(fname), margin=margin, device="cuda")
        assert CR.same_bytes(dev.points, host.points) and CR.same_bytes(dev.length, host.length), fname
        assert ds == hs and hs["moved"] > 0, (fname, ds, hs)


def test_device_wrapper_checks_its_tensors():
    import hgs_runtime as rt
    from scene.strand_collide import resolve_device
    pts, off = CC.flat_strands()
    sdf = CC.field("flat")
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    with pytest.raises(rt.HgsError):
        resolve_device(torch.as_tensor(pts), off_d, sdf)                          # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        resolve_device(pts_d, off_d.to(torch.int32), sdf)
    with pytest.raises(rt.HgsError):
        resolve_device(pts_d.to(torch.float64), off_d, sdf)
    with pytest.raises(rt.HgsError, match="iters"):
        resolve_device(pts_d, off_d, sdf, iters=33)
    with pytest.raises(rt.HgsError, match="margin"):
        resolve_device(pts_d, off_d, sdf, margin=-1.0)


def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    """On device buffers: every refusal returns 1 and leaves the output buffers as they were."""
    import hgs_runtime as rt
    L = rt.lib()
    pts, off = CC.flat_strands()
    sdf = CC.field("flat")
    pts_d, off_d, phi = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda"), sdf.on("cuda")["phi"]
    P, K = pts.shape[0], off.shape[0] - 1
    out = torch.full((P, 3), -7.0, dtype=torch.float32, device="cuda")
    moved = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    unresolved = torch.full((K,), -7, dtype=torch.int32, device="cuda")

    def call(K_=K, P_=P, offsets=off_d.data_ptr(), points=pts_d.data_ptr(), field=phi.data_ptr(), n=sdf.shape, inv_h=1.0, margin=0.0, skin=0.0,
             iters=8, o=out.data_ptr(), m=moved.data_ptr(), u=unresolved.data_ptr()):
        return L.hgs_strand_collide(rt.current_stream(), K_, offsets, P_, points, field, n[0], n[1], n[2], 0.0, 0.0, 0.0, inv_h, margin, skin,
                                    iters, o, m, u)

    nan = float("nan")
    for kw in (dict(K_=-1), dict(P_=-1), dict(iters=0), dict(iters=33), dict(margin=-1.0), dict(margin=nan), dict(skin=-1.0), dict(skin=float("inf")),
               dict(n=(1, 4, 4)), dict(n=(4, 4, 1025)), dict(inv_h=0.0), dict(offsets=None), dict(points=None), dict(field=None), dict(o=None),
               dict(m=None), dict(u=None), dict(o=pts_d.data_ptr())):
        assert call(**kw) == 1 and b"hgs_strand_collide" in L.hgs_last_error(), kw
    assert call(K_=0, P_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((moved == -7).all()) and bool((unresolved == -7).all())
    from scene.strand_collide import default_skin
    assert call(skin=float(default_skin(sdf))) == 0                              # (the case's own skin: the default)
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), moved.cpu().numpy(), unresolved.cpu().numpy()), reference("flat")[:3], "flat")


def test_driver_on_the_device_in_a_child_process(tmp_path):
    """export_strands.py --resolve_head --device cuda as a process of its own, over resampled strands with an interpolated groom, and
    in this process over the joints as they are (ragged), writes the bytes the --device cpu runs write."""
    import export_strands
    model, field = driver_scene(tmp_path)
    script = os.path.join(ROOT, "hair-gs_amd", "export_strands.py")
    for tag, extra in (("groom", ["--points", "20", "--interpolate", "--guides", "3"]), ("joints", ["--points", "0"])):
        common = ["-m", str(model), "--format", "hair", "--format", "usc", "--resolve_head", "--head_sdf", str(field), "--head_margin", "0.002"] + extra
        device = common + ["-o", str(tmp_path / f"dev_{tag}"), "--device", "cuda"]
        if tag == "groom":
            run = subprocess.run([sys.executable, script] + device, capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            line = [t for t in run.stdout.splitlines() if t.startswith("Resolved against the head")]
            assert len(line) == 1 and "moved 0 points" not in line[0]
        else:
            export_strands.main(device)
        export_strands.main(common + ["-o", str(tmp_path / f"host_{tag}"), "--device", "cpu"])
        for ext in (".hair", ".data"):
            d, h = open(tmp_path / (f"dev_{tag}" + ext), "rb").read(), open(tmp_path / (f"host_{tag}" + ext), "rb").read()
            assert len(d) == len(h) and d == h, (tag, ext)
