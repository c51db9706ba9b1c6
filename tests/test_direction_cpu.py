"""The 3-D direction term without a GPU: the numpy path of utils/direction_term.py against the float32 loop of
tests/direction_reference.py (bit for bit) and against its float64 loop (the accuracy bar derived in that module's docstring), the
torch statement loss.losses.strand_direction_loss against both, what the term does to strands that Adam trains with it alone, the
options, train.py's refusals and the binding's surface."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import direction_cases as DC
from tests import direction_reference as DR
from utils import direction_term as D
from utils.trace import Field, save_field


def numpy_path(name, upstream=1.0):
    vol, pts, pairs, min_conf = DC.case(name)
    info = {}
    L, d = D.loss(pts, pairs, vol, min_conf, upstream=upstream, info=info)
    return dict(value=L, d_points=d, **info)


# ---- the numpy path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.NAMES)
def test_numpy_path_equals_the_loop(name):
    got, ref = numpy_path(name), DR.of_case(name)
    for k in ("term", "w", "gs", "d_points"):
        assert got[k].dtype == np.float32 and got[k].tobytes() == ref[k].tobytes(), k
    assert got["active"] == int(ref["active"].sum())
    assert np.float32(got["value"]).tobytes() == np.float32(ref["value"]).tobytes()
    vol, pts, pairs, _ = DC.case(name)
    offsets, entries = D.incidence(pairs, pts.shape[0])
    assert offsets.dtype == np.int32 and entries.dtype == np.int32 and offsets.shape == (pts.shape[0] + 1,) and entries.shape == (2 * pairs.shape[0],)
    flat = pairs.reshape(-1)
    for e in range(min(pts.shape[0], 64)):
        assert entries[offsets[e]:offsets[e + 1]].tolist() == np.nonzero(flat == e)[0].tolist()


def test_hand_made_rows():
    got = numpy_path("hand")
    vol, pts, pairs, _ = DC.case("hand")
    row = {n: i for i, n in enumerate(DC.HAND_ROWS)}
    active = DR.of_case("hand")["active"]
    assert {n for n in DC.HAND_ROWS if not active[row[n]]} == set(DC.HAND_INACTIVE)
    for n in DC.HAND_INACTIVE:
        assert got["term"][row[n]] == 0 and not got["gs"][row[n]].any()
    for n in ("t_equals_top", "below_zero", "nan_endpoint", "inf_endpoint"):
        assert got["w"][row[n]] == 0                                                       # out of range: nothing was loaded
    assert got["w"][row["w_below_gate"]] == np.float32(DC.BELOW) and got["w"][row["w_at_gate"]] == np.float32(DC.MIN_CONF)
    assert got["w"][row["on_a_node"]] == 1 and got["w"][row["cancel"]] == 1
    assert got["term"][row["parallel"]] == 0 and got["term"][row["perpendicular"]] == 1
    assert got["term"][row["parallel_odd"]] in (np.float32(0), np.float32(2.0 ** -24))     # never negative on these inputs
    assert DC.MIN_CONF < got["w"][row["cleared_node"]] < 1 and active[row["cleared_node"]]  # two corners cleared to zeros: they add nothing
    assert (got["term"] >= 0).all() and (got["term"] <= 1).all()
    d = got["d_points"]
    assert not d[0].any()                                                                 # used by no segment
    S = np.float32(pairs.shape[0])
    gs = got["gs"]
    c0, j0 = pairs[row["chain_0"], 0], pairs[row["junction_0"], 0]
    assert d[c0].tobytes() == ((np.float32(0) + -gs[row["chain_0"]]) * (np.float32(1) / S)).tobytes()      # a chain end
    inner = pairs[row["chain_0"], 1]
    assert d[inner].tobytes() == (((np.float32(0) + gs[row["chain_0"]]) + -gs[row["chain_1"]]) * (np.float32(1) / S)).tobytes()
    want = ((np.float32(0) + -gs[row["junction_0"]]) + gs[row["junction_1"]]) + -gs[row["junction_2"]]     # three segments, in (s, side) order
    assert d[j0].tobytes() == (want * (np.float32(1) / S)).tobytes()
    with pytest.raises(ValueError, match="endpoint ids"):
        D.loss(pts, np.array([[0, pts.shape[0]]]), vol, 0.5)
    with pytest.raises(ValueError, match="endpoint ids"):
        D.incidence(np.array([[-1, 0]]), 4)


@pytest.mark.parametrize("name", [n for n in DC.NAMES if n != "hand"])
def test_negated_node_directions_change_no_byte(name):
    """(hand7 holds corners with dot(c, u) == 0 exactly, the one exception of the contract)"""
    vol, pts, pairs, min_conf = DC.case(name)
    rng = np.random.default_rng(17)
    flipped = D.DirectionVolume.__new__(D.DirectionVolume)
    flipped.__dict__.update(vol.__dict__)
    flipped._dev = {}
    flipped.vol = vol.vol.copy()
    flipped.vol[..., :3] *= rng.choice([-1.0, 1.0], size=vol.vol.shape[:3]).astype(np.float32)[..., None]
    assert (flipped.vol != vol.vol).any()
    a, b = {}, {}
    La, da = D.loss(pts, pairs, vol, min_conf, info=a)
    Lb, db = D.loss(pts, pairs, flipped, min_conf, info=b)
    assert La.tobytes() == Lb.tobytes() and da.tobytes() == db.tobytes()
    for k in ("term", "w", "gs"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_volume_packing_and_file(tmp_path):
    vol = DC.volume("hand7")
    assert vol.vol.dtype == np.float32 and vol.vol.shape == (7, 7, 7, 4) and vol.cleared == 2
    assert not vol.vol[6, 6, 6].any() and not vol.vol[5, 6, 6].any() and vol.vol[0, 2, 4, 3] == np.float32(0.5)
    assert vol.inv_h32 == np.float32(8) and vol.origin32.dtype == np.float32 and vol.shape == (7, 7, 7)
    v5 = DC.volume("vol543")
    assert v5.vol.shape == (3, 4, 5, 4) and v5.inv_h32 == np.float32(1.0 / 0.0731)
    f = Field(np.zeros(3), 0.5, (2, 3, 2), np.ones((2, 3, 2, 3)), np.ones((2, 3, 2)))
    save_field(str(tmp_path / "f.npz"), f)
    back = D.DirectionVolume.load(str(tmp_path / "f.npz"))
    assert back.shape == (2, 3, 2) and back.vol.tobytes() == D.DirectionVolume(f).vol.tobytes()
    assert back.on("cpu") is back.on("cpu") and tuple(back.on("cpu")["vol"].shape) == (12, 4)
    np.savez(str(tmp_path / "other.npz"), a=np.zeros(3))
    with open(tmp_path / "junk.npz", "wb") as fh:
        fh.write(b"junk")
    for bad in ("other.npz", "junk.npz", "missing.npz"):
        with pytest.raises(ValueError, match=bad):
            D.DirectionVolume.load(str(tmp_path / bad))
    with pytest.raises(ValueError):
        D.DirectionVolume("f.npz")


# ---- the torch statement ---------------------------------------------------------------------------------------------------
def _model(pts, pairs, dtype=torch.float32):
    return SimpleNamespace(_endpoints=torch.tensor(np.asarray(pts), dtype=dtype).requires_grad_(True), endpoint_pairs=torch.as_tensor(np.asarray(pairs)))


def test_torch_statement_passes_gradcheck_in_float64():
    """A volume that holds one line (with a random sign per node) has no gradient through the lookup position to miss."""
    from loss.losses import strand_direction_loss
    vol = DC.constant((0.3, -0.5, 0.8), flip_seed=4)
    pts, pairs = DC.chains(vol, 24, 9, per=5, step=0.7, spill=0.0)
    pts = np.clip(pts.astype(np.float64), 0.1, 0.9)
    m = _model(pts, pairs, torch.float64)
    assert float(strand_direction_loss(m, vol, 0.5).detach()) > 0.05

    def f(p):
        return strand_direction_loss(SimpleNamespace(_endpoints=p, endpoint_pairs=m.endpoint_pairs), vol, 0.5)
    assert torch.autograd.gradcheck(f, (m._endpoints,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("name", ["swirl_S513", "vol543_S257", "swirl_S16641", "no_segments", "swirl_S0"])
def test_torch_statement_agrees_with_the_numpy_path(name):
    """tests/test_head_sdf_gpu.py's bars between a torch statement and its op: 2e-5 of the value, 2e-4 of the gradient's scale."""
    from loss.losses import strand_direction_loss
    vol, pts, pairs, min_conf = DC.case(name)
    want = numpy_path(name)
    m = _model(pts, pairs)
    L = strand_direction_loss(m, vol, min_conf)
    L.backward()
    print(f"value | strand_direction_loss | {name} | torch {float(L)!r} | numpy {float(want['value'])!r} |")
    assert abs(float(L) - float(want["value"])) <= 2e-5 * abs(float(want["value"]))
    g = m._endpoints.grad.numpy()
    scale = float(np.abs(want["d_points"]).max()) if want["d_points"].size else 0.0
    assert g.shape == want["d_points"].shape and (np.abs(g - want["d_points"]).max() if g.size else 0.0) <= 2e-4 * scale


def test_loss_function_adds_the_term_only_when_on():
    from arguments import OptimizationParams
    from loss import losses as Ls
    from scene.hair_gaussian_model import HairGaussianModel
    strands = _tilted_strands()
    m = HairGaussianModel.from_strands(strands, sh_degree=0, device="cpu", ref_strand_root=strands[:, 0])
    img, cam = torch.rand(3, 8, 8), SimpleNamespace(original_image=torch.rand(3, 8, 8), mask=None)
    opt = OptimizationParams()
    opt.lambda_orientation = opt.lambda_smooth = 0.0
    m.direction_volume = DC.constant()
    _, terms = Ls.loss_function(m, img, cam, opt)
    assert "direction" not in terms                                                       # the volume alone switches nothing on
    opt.lambda_direction = 3.0
    loss, terms = Ls.loss_function(m, img, cam, opt)
    want, _ = D.loss(strands.reshape(-1, 3), m.endpoint_pairs.numpy(), m.direction_volume, 0.5)
    got = float(terms["direction"].detach())
    assert abs(got - float(want)) <= 2e-5 * float(want) and abs(got - np.sin(np.radians(20.0)) ** 2) < 1e-4
    base = max(0, 1.0 - opt.lambda_dssim) * terms["l1"] + opt.lambda_dssim * terms["dssim"]
    assert abs(float(loss.detach()) - float((base + 3.0 * terms["direction"]).detach())) <= 1e-6 * float(loss.detach())
    _, terms = Ls.loss_function(SimpleNamespace(direction_volume=m.direction_volume), img, cam, opt)    # a Stage-I cloud: no term
    assert "direction" not in terms
    del m.direction_volume
    _, terms = Ls.loss_function(m, img, cam, opt)
    assert "direction" not in terms


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.RANDOM + ("hand",))
def test_float32_statement_against_float64(name):
    """|term32 - term64| <= C kappa 2^-23 and max_j |gs32 - gs64| <= C kappa 2^-23 * 2 / |u| over the segments whose gate and eight signs
    agree between the two loops; C = 47 is derived in tests/direction_reference.py.  Worst ratios seen (CPU): 5.4 and 4.5 on
    swirl_S16641, 0.6 and 0.5 on the hand-made rows; no row was left out."""
    rt, rg, n, left_out, gate_differs = DR.accuracy(name)
    S = DC.case(name)[2].shape[0]
    print(f"ratio | direction | {name} | term {rt:.2f} | gs {rg:.2f} | compared {n} | left out {len(left_out)} | gate differs {len(gate_differs)} |")
    assert 17 < DR.C <= 100
    assert rt <= DR.C and rg <= DR.C
    if name == "hand":
        # the rows built to sit on a decision (w at and below the gate, the cancelling and the perpendicular corners) do so by exact
        # arithmetic in both precisions: they decide alike, and nothing else may differ either
        assert list(left_out) == [] and list(gate_differs) == []
        assert n == len(DC.HAND_ROWS) - len(DC.HAND_INACTIVE)
    else:
        assert len(left_out) <= 1e-3 * S and len(gate_differs) <= 1e-3 * S


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
def _tilted_strands(n=6, seg=8):
    """Straight strands inside const9's box, all 20 degrees off its line (0, 0, 1), tilted towards different sides."""
    out = []
    for k in range(n):
        az = 2.0 * np.pi * k / n
        t = np.radians(20.0)
        d = np.array([np.sin(t) * np.cos(az), np.sin(t) * np.sin(az), np.cos(t)])
        root = np.array([0.35 + 0.06 * k, 0.65 - 0.05 * k, 0.25])
        out.append(root[None, :] + 0.05 * np.arange(seg + 1)[:, None] * d[None, :])
    return np.asarray(out, np.float32)


def _mean_angle(m):
    p = m._endpoints.detach().numpy().astype(np.float64)
    u = p[m.endpoint_pairs[:, 1].numpy()] - p[m.endpoint_pairs[:, 0].numpy()]
    return float(np.degrees(np.arccos(np.clip(np.abs(u[:, 2]) / np.linalg.norm(u, axis=1), 0, 1))).mean())


def test_training_with_the_term_alone_turns_the_strands():
    from arguments import OptimizationParams
    from loss import losses as Ls
    from scene.hair_gaussian_model import HairGaussianModel
    img, cam = torch.rand(3, 8, 8), SimpleNamespace(original_image=torch.rand(3, 8, 8), mask=None)
    ends = {}
    for lam in (1.0, 0.0):
        strands = _tilted_strands()
        m = HairGaussianModel.from_strands(strands, sh_degree=0, device="cpu", ref_strand_root=strands[:, 0])
        m.direction_volume = DC.constant()
        opt = OptimizationParams()
        opt.lambda_orientation = opt.lambda_smooth = 0.0
        opt.lambda_direction = lam
        adam = torch.optim.Adam([m._endpoints], lr=1e-3)
        start = _mean_angle(m)
        assert abs(start - 20.0) < 1e-3
        for _ in range(300):
            adam.zero_grad()
            loss, terms = Ls.loss_function(m, img, cam, opt)
            assert ("direction" in terms) == (lam > 0)
            if loss.requires_grad:
                loss.backward()
                adam.step()
        ends[lam] = (_mean_angle(m), m._endpoints.detach().numpy().copy(), strands.reshape(-1, 3))
    print(f"behaviour | mean angle 20.000 -> {ends[1.0][0]:.3f} degrees with the term | {ends[0.0][0]:.3f} without |")
    assert ends[1.0][0] < 10.0
    assert ends[0.0][1].tobytes() == ends[0.0][2].tobytes()                               # off: the strands stay where they were


# ---- options, driver, binding ----------------------------------------------------------------------------------------------
def test_options_default_to_off_and_parse():
    from argparse import ArgumentParser
    from arguments import OptimizationParams
    op = OptimizationParams()
    assert op.lambda_direction == 0 and op.direction_field == "" and op.direction_min_conf == 0.5
    assert [f[0] for f in OptimizationParams.FIELDS[-3:]] == ["lambda_direction", "direction_field", "direction_min_conf"]
    parser = ArgumentParser()
    got = OptimizationParams(parser).extract(parser.parse_args(["--lambda_direction", "0.25", "--direction_field", "f.npz", "--direction_min_conf", "0.75"]))
    assert got.lambda_direction == 0.25 and got.direction_field == "f.npz" and got.direction_min_conf == 0.75


def test_train_without_a_usable_field_names_the_tool(tmp_path):
    import train as train_cli
    out = tmp_path / "out"
    with pytest.raises(SystemExit, match=r"^train\.py: --lambda_direction.*--direction_field.*trace_strands\.py --field"):
        train_cli.main(["-s", str(tmp_path), "-m", str(out), "--lambda_direction", "1"])
    with pytest.raises(SystemExit, match=r"^train\.py: .*trace_strands\.py --field"):
        train_cli.main(["-s", str(tmp_path), "-m", str(out), "--lambda_direction", "1", "--direction_field", str(tmp_path / "missing.npz")])
    with open(tmp_path / "junk.npz", "wb") as fh:
        fh.write(b"junk")
    with pytest.raises(SystemExit, match=r"^train\.py: .*not a direction volume.*trace_strands\.py --field"):
        train_cli.main(["-s", str(tmp_path), "-m", str(out), "--lambda_direction", "1", "--direction_field", str(tmp_path / "junk.npz")])
    assert not os.path.exists(out)                                                        # (refused before anything is written)


def test_binding_symbols_and_refusals():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    want = {"hgs_direction_loss_num_blocks": 1, "hgs_direction_loss_forward": 18, "hgs_direction_loss_backward": 8}
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "hgs.h")) as fh:
        header = fh.read()
    for name, n_args in want.items():
        assert hasattr(L, name) and len(rt.SIGNATURES[name][1]) == n_args
        decl = header[header.rindex(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args, name
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15 and "#define HGS_ABI_VERSION 15" in header
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16                                             # (never dereferenced: every call below is refused first)

    def fwd(S=4, pts=p, pairs=p, vol=p, n=(4, 4, 4), o=(0.0, 0.0, 0.0), k=10.0, mc=0.5, gs=p, term=None, w=None, partials=p, out=p):
        assert L.hgs_direction_loss_forward(None, S, pts, pairs, vol, n[0], n[1], n[2], o[0], o[1], o[2], k, mc, gs, term, w, partials, out) != 0
        return L.hgs_last_error().decode()

    def bwd(E=4, S=4, offsets=p, entries=p, gs=p, up=p, d=p):
        assert L.hgs_direction_loss_backward(None, E, S, offsets, entries, gs, up, d) != 0
        return L.hgs_last_error().decode()
    assert "segments" in fwd(S=-1) and "segments" in fwd(S=(1 << 28) + 1)
    for n in ((1, 4, 4), (4, 1025, 4), (4, 4, -1), (1024, 1024, 65)):
        assert "a grid of" in fwd(n=n)
    for k in (0.0, -1.0, float("inf"), float("nan")):
        assert "1/h" in fwd(k=k)
    assert "min_conf" in fwd(mc=float("nan")) and "min_conf" in fwd(mc=float("inf")) and "origin" in fwd(o=(0.0, float("inf"), 0.0))
    for kw in (dict(pts=None), dict(pairs=None), dict(gs=None), dict(partials=None), dict(vol=None), dict(out=None)):
        assert fwd(**kw).endswith("are required")
    assert "aligned" in fwd(vol=p + 4)
    assert "segments" in bwd(E=-1) and "segments" in bwd(S=-1) and "segments" in bwd(E=(1 << 28) + 1)
    for kw in (dict(offsets=None), dict(entries=None), dict(gs=None), dict(up=None), dict(d=None)):
        assert bwd(**kw).endswith("are required")
    assert L.hgs_direction_loss_backward(None, 0, 0, None, None, None, None, None) == 0   # E == 0 launches nothing
    assert [L.hgs_direction_loss_num_blocks(S) for S in (-1, 0, 1, 256, 257, 16641)] == [0, 0, 1, 1, 2, 66]
    from hgs_runtime.fused import DirectionTable, direction_loss
    with pytest.raises(rt.HgsError):
        DirectionTable(torch.zeros((3, 2), dtype=torch.int64), 4)                         # CPU tensors: there is no CPU path
    with pytest.raises(rt.HgsError):
        direction_loss(torch.zeros(4, 3), None, DC.volume("vol2"), 0.5)
