"""The root attachment on the GPU (csrc/hgs_attach.hip through scene/strand_attach.py): both kernels against the numpy path and the
loop restatement of the contract (tests/attach_reference.py) bit for bit on the hard cases, strand counts and point counts of
tests/attach_cases.py, with and without a direction volume, a second launch and a side stream, the wrappers' checks, the C entry
points' refusals on device buffers, the entry point on both devices, and the driver in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attach_cases as AC
from tests import attach_reference as AR
from tests.test_attach_cpu import (REJOINED, as_strands, assert_same, case_inputs, counted_slice, driver_volume, landing_result, march_reference, masked,
                                   rejoin_reference)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _on(stream, call):
    if stream is None:
        return call()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        res = call()
    stream.synchronize()
    return res


def _march(pts, off, sdf, vol, knobs, stream=None):
    """(device tensors of the march, the same as host arrays with the unspecified rows of ext zeroed)."""
    from scene.strand_attach import attach_device, volume_on
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    dev = _on(stream, lambda: attach_device(pts_d, off_d, sdf, volume_on(vol, "cuda"), **knobs))
    return dev, masked(tuple(t.cpu().numpy() for t in dev))


def _rejoin(pts, attrs, off, march_dev, count, reason, M, stream=None):
    from scene.strand_attach import out_sizes, rejoin_device
    _, out_off = out_sizes(off, count, reason, M)
    t = [torch.as_tensor(v, device="cuda") for v in (pts, attrs, off, out_off)]
    out, oat = _on(stream, lambda: rejoin_device(t[0], t[1], t[2], march_dev[0], march_dev[1], march_dev[2], M, t[3], int(out_off[-1])))
    return out.cpu().numpy(), oat.cpu().numpy(), out_off


@pytest.mark.parametrize("name", AC.HARD_NAMES)
def test_kernels_match_the_numpy_path_and_the_restatement(name):
    from scene.strand_attach import attach_numpy, rejoin_numpy
    c, sdf, vol = case_inputs(name)
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    dev, got = _march(pts, off, sdf, vol, c["knobs"])
    host = attach_numpy(pts, off, sdf, vol, **c["knobs"])
    assert_same(got, host, name + " (numpy)")
    assert_same(got, march_reference(name), name + " (loop)")
    for M in AC.MS:
        joined = _rejoin(pts, attrs, off, dev, got[1], got[2], M)
        assert_same(joined, rejoin_numpy(pts, attrs, off, *host[:3], M), f"{name} M={M} (numpy)", REJOINED)
        assert_same(joined, rejoin_reference(name, M), f"{name} M={M} (loop)", REJOINED)


@pytest.mark.parametrize("K", AC.KS)
def test_kernels_at_every_strand_count(K):
    pts, attrs, off = AC.first_strands(*AC.sphere_strands(), K)
    dev, got = _march(pts, off, AC.field(AC.COUNTED["field"]), AC.volume(AC.COUNTED["volume"]), AC.COUNTED["knobs"])
    for M in AC.MS:
        m, r = counted_slice(K, M)
        assert_same(got, m, f"K={K}")
        assert_same(_rejoin(pts, attrs, off, dev, got[1], got[2], M), r, f"K={K} M={M}", REJOINED)


def test_kernels_with_and_without_a_volume():
    """The same strands and knobs with no volume, with one, with one that has no data, and with entries negated."""
    from scene.strand_attach import attach_numpy
    c, sdf, _ = case_inputs("scene_swirl")
    got = {}
    for vname in (None, "swirl", "zero", "flip", "const"):
        vol = AC.volume(vname) if vname else None
        _, got[vname] = _march(c["points"], c["offsets"], sdf, vol, c["knobs"])
        assert_same(got[vname], attach_numpy(c["points"], c["offsets"], sdf, vol, **c["knobs"]), str(vname))
    assert_same(got[None], got["zero"], "no data steers nothing")
    assert_same(got["swirl"], got["flip"], "negated entries")
    assert not AR.same_bytes(got["swirl"][0], got[None][0]) and not AR.same_bytes(got["swirl"][0], got["const"][0])


def test_kernel_on_the_analytic_head():
    from scene.strand_attach import REACHED
    pts, _, off = AC.landing_strands()
    for grid in AC.LANDING_GRIDS:
        for margin, pull in ((0.0, 0.0), (0.02, 1.0), (0.0, 4.0)):
            _, got = _march(pts, off, AC.field(f"sphere{grid}"), None, dict(margin=margin, pull=pull))
            assert_same(got, landing_result(grid, margin, pull), f"grid={grid} margin={margin} pull={pull}")
            assert (got[2] == REACHED).all()


def test_two_runs_and_a_side_stream_give_equal_bytes():
    c, sdf, vol = case_inputs("special_sphere24_m0.02_swirl_pull0.5")
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    dev, first = _march(pts, off, sdf, vol, c["knobs"])
    joined = _rejoin(pts, attrs, off, dev, first[1], first[2], 100)
    assert_same(_march(pts, off, sdf, vol, c["knobs"])[1], first, "second run")
    side = torch.cuda.Stream()
    dev2, again = _march(pts, off, sdf, vol, c["knobs"], side)
    assert_same(again, first, "side stream")
    assert_same(_rejoin(pts, attrs, off, dev, first[1], first[2], 100), joined, "second rejoin", REJOINED)
    assert_same(_rejoin(pts, attrs, off, dev2, first[1], first[2], 100, side), joined, "side stream rejoin", REJOINED)
    assert first[1].sum() > 20


def test_attach_roots_on_the_device_equals_the_numpy_path():
    """The product's entry point on both devices: every output and every figure of the report; batches and the scalp test included."""
    from scene.strand_attach import REACHED, attach_roots
    for name, M, extra in (("scene_swirl", 0, {}), ("scene_swirl", 7, dict(budget=24 * 257 * 7)), ("special_sphere9_m0.05_swirl", 0, {}),
                           ("special_sphere24_m0.0_const_pull0.0_descent0.5", 100, {}), ("slab_margin", 3, {}), ("no_strands", 0, {}),
                           ("empty_strands_only", 5, {})):
        c, sdf, vol = case_inputs(name)
        strands = as_strands(c["points"], c["attrs"], c["offsets"])
        if name == "scene_swirl":
            ext, count, reason, _ = march_reference(name)
            hit = np.nonzero(reason == REACHED)[0]
            landed = ext[hit, count[hit] - 1]
            extra = dict(extra, scalp_points=landed[landed[:, 2] > 0.0], scalp_distance=1e-3)
        host, hs = attach_roots(strands, sdf, vol, points=M, **extra, **c["knobs"])
        dev, ds = attach_roots(strands, sdf, vol, points=M, device="cuda", **extra, **c["knobs"])
        for what, a, b in zip(("points", "attrs", "offsets", "strand_ids", "length"), dev, host):
            assert AR.same_bytes(np.asarray(a), np.asarray(b)), (name, what)
        assert AR.same_bytes(ds.pop("reason"), hs.pop("reason")) and ds == hs, (name, ds, hs)
        if name == "scene_swirl":
            assert hs["attached"] > 10 and hs["failed"]["off_scalp"] > 10


def test_device_wrappers_check_their_tensors():
    import hgs_runtime as rt
    from scene.strand_attach import attach_device, rejoin_device, volume_on
    c, sdf, vol = case_inputs("tiny")
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    pts_d, att_d, off_d = (torch.as_tensor(v, device="cuda") for v in (pts, attrs, off))
    with pytest.raises(rt.HgsError):
        attach_device(torch.as_tensor(pts), off_d, sdf)                           # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        attach_device(pts_d, off_d.to(torch.int32), sdf)
    with pytest.raises(rt.HgsError):
        attach_device(pts_d.to(torch.float64), off_d, sdf)
    with pytest.raises(rt.HgsError, match="max_steps"):
        attach_device(pts_d, off_d, sdf, max_steps=1025)
    with pytest.raises(rt.HgsError, match="descent"):
        attach_device(pts_d, off_d, sdf, descent=0.0)
    v = volume_on(AC.volume("swirl"), "cuda")
    with pytest.raises(rt.HgsError):
        attach_device(pts_d, off_d, sdf, (v[0][:-1].contiguous(), v[1], v[2], v[3], v[4]))          # fewer nodes than the grid
    with pytest.raises(rt.HgsError):
        attach_device(pts_d, off_d, sdf, (v[0].to(torch.float32), v[1], v[2], v[3], v[4]))
    ext, count, reason, _ = attach_device(pts_d, off_d, sdf, **c["knobs"])
    out_off = torch.as_tensor(np.array([0, 2, 4, 6]), device="cuda")
    for kw in (dict(points=torch.as_tensor(pts)), dict(attrs=att_d[:-1]), dict(ext=ext.to(torch.float32)), dict(ext=ext[:2]), dict(count=count.to(torch.int64)),
               dict(reason=reason[:2]), dict(M=1), dict(out_offsets=out_off[:-1]), dict(n_out=-1)):
        args = dict(points=pts_d, attrs=att_d, offsets=off_d, ext=ext, count=count, reason=reason, M=0, out_offsets=out_off, n_out=6)
        args.update(kw)
        with pytest.raises(rt.HgsError):
            rejoin_device(**args)


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """On device buffers: every refusal returns 1 and leaves the output buffers as they were; a strand whose output range is not the
    size the rejoin asks for is not written."""
    import hgs_runtime as rt
    from scene.strand_attach import default_tol, out_sizes
    L = rt.lib()
    c, sdf, _ = case_inputs("tiny")
    pts, attrs, off = c["points"], c["attrs"], c["offsets"]
    pts_d, att_d, off_d, phi = torch.as_tensor(pts, device="cuda"), torch.as_tensor(attrs, device="cuda"), torch.as_tensor(off, device="cuda"), sdf.on("cuda")["phi"]
    vol = AC.volume("swirl")
    vdir, vconf = torch.from_numpy(vol.dir).cuda(), torch.from_numpy(vol.conf).cuda()
    P, K, rows = pts.shape[0], off.shape[0] - 1, 9
    ext = torch.full((K, rows, 3), -7.0, dtype=torch.float64, device="cuda")
    count, reason = (torch.full((K,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    landed = torch.full((K,), -7.0, dtype=torch.float32, device="cuda")
    inf, nan = float("inf"), float("nan")

    def attach(K_=K, P_=P, offsets=off_d.data_ptr(), points=pts_d.data_ptr(), field=phi.data_ptr(), n=sdf.shape, inv_h=1.0, vd=None, vc=None, vn=vol.shape,
               vh=vol.spacing, min_conf=0.5, margin=0.0, tol=float(default_tol(sdf)), step=0.2, max_steps=rows - 1, land_iters=4, pull=0.0, descent=0.25,
               max_distance=inf, e=ext.data_ptr(), cn=count.data_ptr(), r=reason.data_ptr(), ld=landed.data_ptr()):
        return L.hgs_root_attach(rt.current_stream(), K_, offsets, P_, points, field, n[0], n[1], n[2], 0.0, 0.0, 0.0, inv_h, vd, vc, vn[0], vn[1], vn[2],
                                 float(vol.origin[0]), float(vol.origin[1]), float(vol.origin[2]), vh, min_conf, margin, tol, step, max_steps, land_iters, pull,
                                 descent, max_distance, e, cn, r, ld)

    for kw in (dict(K_=-1), dict(P_=-1), dict(max_steps=0), dict(max_steps=1025), dict(land_iters=0), dict(land_iters=9), dict(margin=-1.0), dict(margin=nan),
               dict(tol=-1.0), dict(tol=inf), dict(step=0.0), dict(step=nan), dict(pull=-1.0), dict(descent=0.0), dict(descent=1.5), dict(max_distance=-1.0),
               dict(max_distance=nan), dict(n=(1, 2, 2)), dict(n=(2, 2, 1025)), dict(inv_h=0.0), dict(vd=vdir.data_ptr()), dict(vc=vconf.data_ptr()),
               dict(vd=vdir.data_ptr(), vc=vconf.data_ptr(), vn=(1, 7, 7)), dict(vd=vdir.data_ptr(), vc=vconf.data_ptr(), vh=0.0),
               dict(vd=vdir.data_ptr(), vc=vconf.data_ptr(), min_conf=nan), dict(offsets=None), dict(points=None), dict(field=None), dict(e=None), dict(cn=None),
               dict(r=None), dict(ld=None), dict(e=pts_d.data_ptr()), dict(e=phi.data_ptr()), dict(r=count.data_ptr()), dict(ld=pts_d.data_ptr())):
        assert attach(**kw) == 1 and b"hgs_root_attach" in L.hgs_last_error(), kw
    assert attach(K_=0, P_=0) == 0
    torch.cuda.synchronize()
    assert bool((ext == -7.0).all()) and bool((count == -7).all()) and bool((reason == -7).all()) and bool((landed == -7.0).all())
    assert attach() == 0                                                          # (the case's own knobs, max_steps = 8)
    torch.cuda.synchronize()
    want = AR.march(pts, off, sdf, None, step=0.2, pull=0.0, max_steps=rows - 1)
    got = masked((ext.cpu().numpy(), count.cpu().numpy(), reason.cpu().numpy(), landed.cpu().numpy()))
    assert_same(got, want, "tiny through the entry point")

    reached, out_off = out_sizes(off, got[1], got[2], 0)
    n_out = int(out_off[-1])
    out_off_d = torch.as_tensor(out_off, device="cuda")
    out = torch.full((n_out, 3), -7.0, dtype=torch.float32, device="cuda")
    oat = torch.full((n_out, attrs.shape[1]), -7.0, dtype=torch.float32, device="cuda")

    def rejoin(K_=K, P_=P, offsets=off_d.data_ptr(), points=pts_d.data_ptr(), at=att_d.data_ptr(), C_=attrs.shape[1], e=ext.data_ptr(), rows_=rows,
               cn=count.data_ptr(), r=reason.data_ptr(), M=0, oo=out_off_d.data_ptr(), n=n_out, o=out.data_ptr(), oa=oat.data_ptr()):
        return L.hgs_strand_rejoin(rt.current_stream(), K_, offsets, P_, points, at, C_, e, rows_, cn, r, M, oo, n, o, oa)

    for kw in (dict(K_=-1), dict(P_=-1), dict(n=-1), dict(C_=-1), dict(C_=65), dict(M=1), dict(M=-1), dict(rows_=1), dict(rows_=1026), dict(offsets=None),
               dict(points=None), dict(at=None), dict(e=None), dict(cn=None), dict(r=None), dict(oo=None), dict(o=None), dict(oa=None), dict(o=pts_d.data_ptr()),
               dict(o=ext.data_ptr()), dict(oa=att_d.data_ptr()), dict(oa=out.data_ptr())):
        assert rejoin(**kw) == 1 and b"hgs_strand_rejoin" in L.hgs_last_error(), kw
    assert rejoin(K_=0) == 0
    assert rejoin(M=100) == 0                                                     # the reached strands own count + n rows, not 100: they are not written
    torch.cuda.synchronize()
    for s in range(K):
        rows_s = slice(int(out_off[s]), int(out_off[s + 1]))
        if reached[s]:
            assert bool((out[rows_s] == -7.0).all()) and bool((oat[rows_s] == -7.0).all()), s
        else:
            assert AR.same_bytes(out[rows_s].cpu().numpy(), pts[off[s]:off[s + 1]]), s
    assert reached.sum() >= 1
    assert rejoin() == 0
    torch.cuda.synchronize()
    assert_same((out.cpu().numpy(), oat.cpu().numpy(), out_off), AR.rejoin(pts, attrs, off, *want[:3], 0), "tiny rejoined through the entry point", REJOINED)


def test_driver_on_the_device_in_a_child_process(tmp_path):
    """export_strands.py --attach_roots --device cuda as a process of its own, steered, over resampled strands with an interpolated groom
    and the push-out behind it, and in this process over the joints as they are (ragged), writes the bytes the --device cpu runs write."""
    import export_strands
    from tests.test_collide_cpu import driver_scene
    from utils import head_sdf
    model, field = driver_scene(tmp_path)
    volume = driver_volume(tmp_path, head_sdf.load_sdf(str(field)))
    script = os.path.join(ROOT, "hair-gs_amd", "export_strands.py")
    for tag, extra in (("groom", ["--points", "20", "--interpolate", "--guides", "3", "--resolve_head", "--attach_field", str(volume), "--attach_pull", "0.5"]),
                       ("joints", ["--points", "0", "--attach_margin", "0.002", "--attach_scalp_distance", "0.05"])):
        common = ["-m", str(model), "--format", "hair", "--format", "usc", "--attach_roots", "--head_sdf", str(field)] + extra
        device = common + ["-o", str(tmp_path / f"dev_{tag}"), "--device", "cuda"]
        if tag == "groom":
            run = subprocess.run([sys.executable, script] + device, capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            line = [t for t in run.stdout.splitlines() if t.startswith("Attached to the head")]
            assert len(line) == 1 and "0 of 7 strands attached" not in line[0] and "steered by" in line[0]
        else:
            export_strands.main(device)
        export_strands.main(common + ["-o", str(tmp_path / f"host_{tag}"), "--device", "cpu"])
        for ext in (".hair", ".data"):
            d, h = open(tmp_path / (f"dev_{tag}" + ext), "rb").read(), open(tmp_path / (f"host_{tag}" + ext), "rb").read()
            assert len(d) == len(h) and d == h, (tag, ext)
