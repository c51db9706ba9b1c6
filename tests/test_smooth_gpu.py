"""The strand smoothing on the GPU (csrc/hgs_strand_smooth.hip through scene/strand_smooth.py): the kernel against the numpy path and
the loop restatement of the contract (tests/smooth_reference.py) bit for bit on the hard cases and strand counts of
tests/smooth_cases.py, a second launch and a side stream, the entry point on both devices, the wrapper's checks, the C entry point's
refusals on device buffers, and the driver in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import smooth_cases as SC
from tests import smooth_reference as SR
from tests.test_smooth_cpu import assert_same, pool_reference, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _device(pts, off, params, stream=None, **kw):
    from scene.strand_smooth import smooth_device
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    if stream is None:
        res = smooth_device(pts_d, off_d, *params, **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            res = smooth_device(pts_d, off_d, *params, **kw)
        stream.synchronize()
    return tuple(t.cpu().numpy() for t in res)


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_kernel_matches_the_numpy_path_and_the_restatement(name):
    from scene.strand_smooth import smooth_numpy
    pts, off, params = SC.hard_cases()[name]
    got = _device(pts, off, params)
    assert_same(got, smooth_numpy(pts, off, *params), name + " (numpy)")
    assert_same(got, reference(name), name + " (loop)")


@pytest.mark.parametrize("K", SC.KS)
def test_kernel_at_every_strand_count(K):
    pts, off = SC.first_strands(*SC.pool_strands(), K)
    ref = pool_reference()
    assert_same(_device(pts, off, SC.DEFAULTS), (ref[0][:off[K]], ref[1][:K], ref[2][:K]), f"K={K}")


def test_every_workgroup_shape_gives_the_same_bytes():
    """The LDS slice, and with it the wavefronts a workgroup holds (4, 2, 1), follows max_joints: the pool's strands (at most 140
    joints) give the same bytes in slices of 140, 409 (the last with four wavefronts), 410, 819 (the last with two), 820 and 1024."""
    from scene.strand_smooth import longest_eligible
    pts, off = SC.pool_strands()
    ref = pool_reference()
    assert longest_eligible(off) == 140
    for slot in (None, 140, 409, 410, 819, 820, 1024):
        assert_same(_device(pts, off, SC.DEFAULTS, max_joints=slot), ref, f"max_joints={slot}")


def test_two_runs_and_a_side_stream_give_equal_bytes():
    pts, off, params = SC.hard_cases()["edges_move"]
    first = _device(pts, off, params)
    assert_same(_device(pts, off, params), first, "second run")
    assert_same(_device(pts, off, params, torch.cuda.Stream()), first, "side stream")
    assert first[2].sum() > 0


def test_smooth_strands_on_the_device_equals_the_numpy_path():
    """The product's entry point on both devices: points, lengths and every figure of the report."""
    from scene.strand_export import StrandExport
    from scene.strand_smooth import smooth_strands
    for (pts, off), kw in ((SC.special_strands(), dict(max_move=SC.ZIGZAG_MOVE)), (SC.edge_strands(), dict()), (SC.pool_strands(), dict(iters=3, mu=0.0))):
        K = off.shape[0] - 1
        strands = StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), off, np.arange(K, dtype=np.int64), np.zeros(K))
        host, hs = smooth_strands(strands, **kw)
        dev, ds = smooth_strands(strands, device="cuda", **kw)
        assert SR.same_bytes(dev.points, host.points) and SR.same_bytes(dev.length, host.length), kw
        assert ds == hs and hs["smoothed"] > 0, (ds, hs)


def test_device_wrapper_checks_its_tensors():
    import hgs_runtime as rt
    from scene.strand_smooth import smooth_device
    pts, off = SC.special_strands()
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    with pytest.raises(rt.HgsError):
        smooth_device(torch.as_tensor(pts), off_d)                                 # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        smooth_device(pts_d, off_d.to(torch.int32))
    with pytest.raises(rt.HgsError):
        smooth_device(pts_d.to(torch.float64), off_d)
    for params, words in SC.REFUSED:
        with pytest.raises(rt.HgsError, match=words):
            smooth_device(pts_d, off_d, *params)
    with pytest.raises(rt.HgsError, match="max_joints"):
        smooth_device(pts_d, off_d, max_joints=1025)


def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    """On device buffers: every refusal returns 1 and leaves the output buffers as they were."""
    import hgs_runtime as rt
    from scene.strand_smooth import longest_eligible
    L = rt.lib()
    pts, off, params = SC.hard_cases()["special_move"]
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    P, K = pts.shape[0], off.shape[0] - 1
    out = torch.full((P, 3), -7.0, dtype=torch.float32, device="cuda")
    status = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    clamped = torch.full((K,), -7, dtype=torch.int32, device="cuda")

    def call(K_=K, P_=P, offsets=off_d.data_ptr(), points=pts_d.data_ptr(), slot=longest_eligible(off), iters=params[0], lam=params[1], mu=params[2],
             has=1, move=params[3], o=out.data_ptr(), s=status.data_ptr(), c=clamped.data_ptr()):
        return L.hgs_strand_smooth(rt.current_stream(), K_, offsets, P_, points, slot, iters, lam, mu, has, move, o, s, c)

    nan = float("nan")
    for kw in (dict(K_=-1), dict(P_=-1), dict(slot=-1), dict(slot=1025), dict(iters=0), dict(iters=257), dict(lam=0.0), dict(lam=1.5), dict(lam=nan),
               dict(lam=1.0, mu=-1.0), dict(mu=-0.5), dict(mu=0.3), dict(mu=nan), dict(lam=0.9, mu=-1.0), dict(move=0.0), dict(move=-1.0),
               dict(move=float("inf")), dict(move=nan), dict(offsets=None), dict(points=None), dict(o=None), dict(s=None), dict(c=None),
               dict(o=pts_d.data_ptr()), dict(c=status.data_ptr())):
        assert call(**kw) == 1 and b"hgs_strand_smooth" in L.hgs_last_error(), kw
    assert call(K_=0, P_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((status == -7).all()) and bool((clamped == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), status.cpu().numpy(), clamped.cpu().numpy()), reference("special_move"), "special_move")


def test_driver_on_the_device_in_a_child_process(tmp_path):
    """export_strands.py --smooth_strands --device cuda as a process of its own, over resampled strands in the whole chain, and in this
    process over the joints as they are (ragged), writes the bytes the --device cpu runs write."""
    import export_strands
    from tests.test_collide_cpu import driver_scene
    model, field = driver_scene(tmp_path)
    script = os.path.join(ROOT, "hair-gs_amd", "export_strands.py")
    for tag, extra in (("chain", ["--points", "20", "--head_sdf", str(field), "--attach_roots", "--interpolate", "--guides", "3", "--resolve_head"]),
                       ("joints", ["--points", "0", "--smooth_max_move", "2e-4"])):
        common = ["-m", str(model), "--format", "hair", "--format", "usc", "--smooth_strands"] + extra
        device = common + ["-o", str(tmp_path / f"dev_{tag}"), "--device", "cuda"]
        if tag == "chain":
            run = subprocess.run([sys.executable, script] + device, capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            line = [t for t in run.stdout.splitlines() if t.startswith("Smoothed strands")]
            assert len(line) == 1 and " 0 of " not in line[0]
        else:
            export_strands.main(device)
        export_strands.main(common + ["-o", str(tmp_path / f"host_{tag}"), "--device", "cpu"])
        for ext in (".hair", ".data"):
            d, h = open(tmp_path / (f"dev_{tag}" + ext), "rb").read(), open(tmp_path / (f"host_{tag}" + ext), "rb").read()
            assert len(d) == len(h) and d == h, (tag, ext)
