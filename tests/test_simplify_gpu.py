"""The strand simplification on the GPU (csrc/hgs_strand_simplify.hip through scene/strand_simplify.py): the kernel against the numpy
path and the recursive restatement of the contract (tests/simplify_reference.py) bit for bit on the hard cases and strand counts of
tests/simplify_cases.py, every workgroup shape, a second launch and a side stream, the entry point on both devices, the wrapper's
checks, the C entry point's refusals on device buffers, and the driver in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import simplify_cases as SC
from tests import simplify_reference as SR
from tests.test_simplify_cpu import DRIVER_TOL, assert_same, cut, export_of, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _device(pts, off, tol, stream=None, **kw):
    from scene.strand_simplify import simplify_device
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    if stream is None:
        res = simplify_device(pts_d, off_d, tol, **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            res = simplify_device(pts_d, off_d, tol, **kw)
        stream.synchronize()
    return tuple(t.cpu().numpy() for t in res)


@pytest.mark.parametrize("name", SC.HARD_NAMES)
def test_kernel_matches_the_numpy_path_and_the_restatement(name):
    from scene.strand_simplify import simplify_numpy
    pts, off, tol = SC.hard_cases()[name]
    got = _device(pts, off, tol)
    assert_same(got, simplify_numpy(pts, off, tol), name + " (numpy)")
    assert_same(got, reference(name), name + " (recursion)")


@pytest.mark.parametrize("K", SC.KS)
def test_kernel_at_every_strand_count(K):
    pts, off, tol = SC.hard_cases()["pool"]
    p, o = SC.first_strands(pts, off, K)
    assert_same(_device(p, o, tol), cut(reference("pool"), off, K), f"K={K}")


def test_every_workgroup_shape_gives_the_same_bytes():
    """The LDS slice (48 * max_joints + 128 bytes), and with it the wavefronts a workgroup holds (4 up to 338 joints, 2 up to 680, then
    1), follows max_joints: the pool's strands (at most 140 joints) give the same bytes in every slice of SC.SLOTS."""
    from scene.strand_smooth import longest_eligible
    pts, off, tol = SC.hard_cases()["pool"]
    assert longest_eligible(off) == 140
    for slot in SC.SLOTS:
        assert_same(_device(pts, off, tol, max_joints=slot), reference("pool"), f"max_joints={slot}")


def test_a_strand_longer_than_the_slice_is_long():
    pts, off, tol = SC.hard_cases()["pool"]
    keep, status, rounds = _device(pts, off, tol, max_joints=100)
    n = off[1:] - off[:-1]
    ref = reference("pool")
    over = n > 100
    assert over.sum() > 50 and (status[over] == 2).all() and not rounds[over].any() and all(keep[off[s]:off[s + 1]].all() for s in np.nonzero(over)[0])
    assert SR.same_bytes(status[~over], ref[1][~over]) and SR.same_bytes(rounds[~over], ref[2][~over])
    keep, status, rounds = _device(pts, off, tol, max_joints=0)
    assert keep.all() and not rounds.any() and status.tolist() == [1 if m < 3 else 2 for m in n]


def test_two_runs_and_a_side_stream_give_equal_bytes():
    """A second launch into the same buffers (filled with other bytes in between: the kernel writes every element), and a side stream."""
    import hgs_runtime as rt
    from scene.strand_smooth import longest_eligible
    pts, off, tol = SC.hard_cases()["edges"]
    first = _device(pts, off, tol)
    assert_same(first, reference("edges"), "first run")
    assert_same(_device(pts, off, tol, torch.cuda.Stream()), first, "side stream")
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    P, K = pts.shape[0], off.shape[0] - 1
    keep = torch.empty(P, dtype=torch.uint8, device="cuda")
    status, rounds = torch.empty(K, dtype=torch.int32, device="cuda"), torch.empty(K, dtype=torch.int32, device="cuda")
    for fill in (0, 77):
        keep.fill_(fill), status.fill_(fill), rounds.fill_(fill)
        rt.check(rt.lib().hgs_strand_simplify(rt.current_stream(), K, off_d.data_ptr(), P, pts_d.data_ptr(), longest_eligible(off), tol,
                                              keep.data_ptr(), status.data_ptr(), rounds.data_ptr()))
        torch.cuda.synchronize()
        assert_same((keep.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()), first, f"buffers filled with {fill}")
    assert 0 < first[0].sum() < P


def test_simplify_strands_on_the_device_equals_the_numpy_path():
    """The product's entry point on both devices: points, attributes, offsets, lengths and every figure of the report."""
    from scene.strand_simplify import simplify_strands
    for name in ("shapes", "edges", "pool", "nonfinite"):
        pts, off, tol = SC.hard_cases()[name]
        attrs = np.random.default_rng(1).normal(size=(pts.shape[0], 5)).astype(np.float32)
        strands = export_of(pts, off, attrs)
        host, hs = simplify_strands(strands, tol)
        dev, ds = simplify_strands(strands, tol, device="cuda")
        for a, b in zip(dev, host):
            assert SR.same_bytes(a, b), name
        assert ds == hs and hs["joints_after"] < hs["joints_before"], (ds, hs)


def test_device_wrapper_checks_its_tensors():
    import hgs_runtime as rt
    from scene.strand_simplify import simplify_device
    pts, off = SC.shape_strands()
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    with pytest.raises(rt.HgsError):
        simplify_device(torch.as_tensor(pts), off_d, 0.5)                          # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        simplify_device(pts_d, off_d.to(torch.int32), 0.5)
    with pytest.raises(rt.HgsError):
        simplify_device(pts_d.to(torch.float64), off_d, 0.5)
    for bad in SC.REFUSED:
        with pytest.raises(rt.HgsError, match="tol"):
            simplify_device(pts_d, off_d, bad)
    for bad in (1025, 2, -1):
        with pytest.raises(rt.HgsError, match="max_joints"):
            simplify_device(pts_d, off_d, 0.5, max_joints=bad)


def test_entry_point_refuses_bad_arguments_and_launches_nothing():
    """On device buffers: every refusal returns 1 and leaves the output buffers as they were."""
    import hgs_runtime as rt
    from scene.strand_smooth import longest_eligible
    L = rt.lib()
    pts, off, tol = SC.hard_cases()["shapes"]
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    P, K = pts.shape[0], off.shape[0] - 1
    keep = torch.full((P,), 77, dtype=torch.uint8, device="cuda")
    status = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    rounds = torch.full((K,), -7, dtype=torch.int32, device="cuda")

    def call(K_=K, P_=P, offsets=off_d.data_ptr(), points=pts_d.data_ptr(), slot=longest_eligible(off), tol_=tol, k=keep.data_ptr(),
             s=status.data_ptr(), r=rounds.data_ptr()):
        return L.hgs_strand_simplify(rt.current_stream(), K_, offsets, P_, points, slot, tol_, k, s, r)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(K_=-1), dict(P_=-1), dict(slot=-1), dict(slot=1), dict(slot=2), dict(slot=1025), dict(tol_=-1.0), dict(tol_=nan), dict(tol_=inf),
               dict(tol_=-inf), dict(offsets=None), dict(points=None), dict(k=None), dict(s=None), dict(r=None), dict(k=pts_d.data_ptr()),
               dict(r=status.data_ptr()), dict(s=off_d.data_ptr())):
        assert call(**kw) == 1 and b"hgs_strand_simplify" in L.hgs_last_error(), kw
    assert call(K_=0, P_=0) == 0
    torch.cuda.synchronize()
    assert bool((keep == 77).all()) and bool((status == -7).all()) and bool((rounds == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert_same((keep.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()), reference("shapes"), "shapes")


def test_driver_on_the_device_in_a_child_process(tmp_path):
    """export_strands.py --simplify --device cuda as a process of its own, at the end of the whole chain with guides chosen, and in this
    process over the joints as they are (ragged), writes the bytes the --device cpu runs write."""
    import export_strands
    from tests.test_collide_cpu import driver_scene
    model, field = driver_scene(tmp_path)
    script = os.path.join(ROOT, "hair-gs_amd", "export_strands.py")
    for tag, extra in (("chain", ["--points", "20", "--head_sdf", str(field), "--attach_roots", "--smooth_strands", "--interpolate", "--guides", "3",
                                  "--resolve_head", "--select_guides", "4", "--select_samples", "4"]),
                       ("joints", ["--points", "0"])):
        common = ["-m", str(model), "--format", "hair", "--format", "usc", "--simplify", DRIVER_TOL] + extra
        device = common + ["-o", str(tmp_path / f"dev_{tag}"), "--device", "cuda"]
        if tag == "chain":
            run = subprocess.run([sys.executable, script] + device, capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            line = [t for t in run.stdout.splitlines() if t.startswith("Simplified strands")]
            assert len(line) == 1 and " 0 of " not in line[0]
        else:
            export_strands.main(device)
        export_strands.main(common + ["-o", str(tmp_path / f"host_{tag}"), "--device", "cpu"])
        names = [f"{tag}{ext}" for ext in (".hair", ".data")] + ([f"{tag}_guides{ext}" for ext in (".hair", ".data")] if tag == "chain" else [])
        for name in names:
            d, h = open(tmp_path / ("dev_" + name), "rb").read(), open(tmp_path / ("host_" + name), "rb").read()
            assert len(d) == len(h) and d == h, name
