"""Strand growth (HairTopologyMixin.growing, reference scene/hair_gaussian_model.py:1098-1200) on the CPU: the host form against
(1) what the reference's own growing() computed on the same models (tests/golden/make_ref_growth_pins.py), bit for bit, and
(2) a per-strand loop restatement of the reference's statements with this project's deviations b and c (attributes from the rows
of the whole segment table, shared tips not grown), on models WITH background segments and shared tips; then the consistency of
the grown model and the no-op."""
import os

import numpy as np
import pytest
import torch

from tests import test_topology_restatement_cpu as T
from arguments import OptimizationParams

GROUPS = ("endpoints", "f_dc", "f_rest", "opacity", "mask", "width")
_PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_growth_pins.npz")


class Info:
    def __init__(self):
        self.densification_info = {}


def growth_model(seed, background=False, device="cpu", num_points_strand=None, k_avg=3):
    """test_topology_restatement_cpu._random_model(seed) (collapsed interior segments, distinct attributes, Adam moments) with
    degree-3 f_rest rows, strands of different lengths (the tips of some cut off), the last segment -- or the last three -- of
    some strands collapsed, and, unless `background`, every segment in the foreground.  num_points_strand None: the longest
    strand's length (those strands are at the limit)."""
    m = T._random_model(seed)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        P = m.endpoint_pairs.shape[0]
        if not background:
            m._mask.copy_(torch.rand((P, 1), generator=g) * 3 + 0.5)
            m._opacity.copy_(torch.randn((P, 1), generator=g) + 1.0)
    rest = torch.randn((P, 15, 3), generator=g) * 0.05
    m._features_rest = torch.nn.Parameter(rest.requires_grad_(True))
    keep = {gr["name"]: dict(m.optimizer.state[gr["params"][0]]) for gr in m.optimizer.param_groups}
    keep["f_rest"] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(rest.shape, generator=g), "exp_avg_sq": torch.rand(rest.shape, generator=g)}
    stats = (m.xyz_gradient_accum, m.denom, m.max_radii2D)
    m.training_setup(OptimizationParams())
    for gr in m.optimizer.param_groups:
        m.optimizer.state[gr["params"][0]] = keep[gr["name"]]
    m.xyz_gradient_accum, m.denom, m.max_radii2D = stats
    m.compute_strands_info()
    si = m.strands_info
    # cut the tips of some strands: strands of different lengths
    seg = np.asarray(si.segment_rows)
    fg = np.nonzero(m.compute_foreground_mask().numpy())[0]
    prune = np.zeros(P, bool)
    for s in range(si.n_strands):
        o0, o1 = int(si.offsets[s]), int(si.offsets[s + 1])
        cut = 2 if s % 5 == 0 else (1 if s % 3 == 0 else 0)
        if o1 - o0 > cut + 1 and cut:
            prune[fg[seg[o1 - cut:o1]]] = True
    if prune.any():
        m.prune_segments(torch.from_numpy(prune))
    m.compute_strands_info()
    si = m.strands_info
    with torch.no_grad():
        for s in range(si.n_strands):
            o0, o1 = int(si.offsets[s]), int(si.offsets[s + 1])
            r = np.asarray(si.rows)[o0:o1]
            if s % 4 == 1:                                   # the last segment collapsed
                m._endpoints[int(r[-1, 1])] = m._endpoints[int(r[-1, 0])]
            elif s % 4 == 2 and o1 - o0 >= 3:                # the last three collapsed
                for a, b in r[-3:].tolist():
                    m._endpoints[b] = m._endpoints[int(r[-3, 0])]
    m.compute_strands_info()
    off = m.strands_info.offsets
    m.training_args.num_points_strand = int(np.diff(off).max()) if num_points_strand is None else num_points_strand
    m.training_args.growth_averaging_points = k_avg
    return to_cuda(m) if device != "cpu" else m


def to_cuda(m):
    """The CPU model `m` moved to the GPU: parameters, Adam moments, statistics, id tables; strands_info walked again there."""
    state = {gr["name"]: dict(m.optimizer.state.get(gr["params"][0], {})) for gr in m.optimizer.param_groups}
    stats = (m.xyz_gradient_accum, m.denom, m.max_radii2D)
    for _, attr in m._PARAM_ATTRS:
        setattr(m, attr, torch.nn.Parameter(getattr(m, attr).detach().cuda().contiguous().requires_grad_(True)))
    m.endpoint_pairs, m.strand_root_endpoint_idx, m.device = m.endpoint_pairs.cuda(), m.strand_root_endpoint_idx.cuda(), "cuda"
    m.training_setup(m.training_args)
    for gr in m.optimizer.param_groups:
        st = state[gr["name"]]
        if st:
            m.optimizer.state[gr["params"][0]] = {"step": st["step"], "exp_avg": st["exp_avg"].cuda(), "exp_avg_sq": st["exp_avg_sq"].cuda()}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = (t.cuda() for t in stats)
    m.compute_strands_info()
    return m


def restated_growth(m, growth_length):
    """The reference's loop (:1112-1178), statement by statement, over this model's strands, with deviations b (the attribute
    rows are the strand's rows of the whole table) and c (a tip another row of the table uses is not grown).  Returns
    (new pairs, endpoints, f_dc, f_rest, opacity, mask, width) as numpy arrays, the grown count and the shared-tip count."""
    ta = m.training_args
    si = m.strands_info
    ep = m._endpoints.detach().cpu().numpy()
    attrs = [getattr(m, a).detach().cpu().numpy() for a in ("_features_dc", "_features_rest", "_opacity", "_mask", "_width")]
    fg = np.nonzero(m.compute_foreground_mask().cpu().numpy())[0]
    pairs_all = m.endpoint_pairs.cpu().numpy()
    deg = np.bincount(pairs_all.reshape(-1))
    out = [[] for _ in range(7)]
    total, counter, shared = ep.shape[0], 0, 0
    for pairs, seg_id in zip(si.list_strands, si.list_strands_segments_id):
        pairs, seg_id = np.asarray(pairs).reshape(-1, 2), fg[np.asarray(seg_id)]
        if pairs.shape[0] >= ta.num_points_strand:
            continue
        tip = ep[pairs[-1, 1]]
        k = min(pairs.shape[0], ta.growth_averaging_points)
        segs, ids = pairs[-k:], seg_id[-k:]
        d = ep[segs[:, 1]] - ep[segs[:, 0]]
        dn = np.linalg.norm(d, axis=1)
        ok = ~(dn < m.min_val)
        segs, d, dn, ids = segs[ok], d[ok], dn[ok], ids[ok]
        if segs.shape[0] == 0:
            continue
        if deg[pairs[-1, 1]] != 1:
            shared += 1
            continue
        d = d / dn[:, np.newaxis]
        if growth_length is None:
            growth_length = np.mean(dn)
        out[0].append([pairs[-1, 1], total + counter])
        out[1].append(tip + np.mean(d, axis=0) * growth_length)
        for i, a in enumerate(attrs):
            out[2 + i].append(np.mean(a[ids], axis=0))
        counter += 1
    shapes = [(2,), (3,)] + [a.shape[1:] for a in attrs]
    res = [np.array(o, dtype=np.int64 if i == 0 else np.float32).reshape((-1,) + tuple(shapes[i])) for i, o in enumerate(out)]
    return res, counter, shared


def grown_rows(m, n_before):
    """The rows growing() appended: pairs, endpoints and the five attribute groups, as numpy arrays."""
    e0 = m._endpoints.shape[0] - (m.endpoint_pairs.shape[0] - n_before)
    return [m.endpoint_pairs[n_before:].cpu().numpy(), m._endpoints.detach()[e0:].cpu().numpy()] + \
        [getattr(m, a).detach()[n_before:].cpu().numpy() for a in ("_features_dc", "_features_rest", "_opacity", "_mask", "_width")]


def assert_consistent_after_growth(m, before, grown):
    """Every group's row count, zero Adam rows for what was appended, strands still chains, every grown strand one segment
    longer with the new endpoint as its tip.  `before`: (pairs, n_endpoints, {tip id: n_seg}) taken before growth."""
    pairs0, n_ep0, tips = before
    P0, P = pairs0.shape[0], m.endpoint_pairs.shape[0]
    assert P == P0 + grown and m._endpoints.shape[0] == n_ep0 + grown
    assert np.array_equal(m.endpoint_pairs[:P0].cpu().numpy(), pairs0)
    for gr in m.optimizer.param_groups:
        p = gr["params"][0]
        n_new, n = (grown, n_ep0 + grown) if gr["name"] == "endpoints" else (grown, P)
        assert p.shape[0] == n, gr["name"]
        st = m.optimizer.state.get(p, {})          # (a model that has taken no Adam step yet holds no moments)
        for mom in ("exp_avg", "exp_avg_sq"):
            if mom not in st:
                continue
            assert st[mom].shape == p.shape and not st[mom][n - n_new:].any(), (gr["name"], mom)
    for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D):
        assert t.shape[0] == P and not t.any()
    deg = np.bincount(m.endpoint_pairs.cpu().numpy().reshape(-1))
    assert deg.max() <= 2
    new = m.endpoint_pairs[P0:].cpu().numpy()
    assert np.array_equal(new[:, 1], np.arange(n_ep0, n_ep0 + grown))
    tip_of = strand_tips(m)
    for old_tip, new_id in new.tolist():
        assert tip_of.get(new_id) == tips[old_tip] + 1, (old_tip, new_id)


def strand_tips(m):
    si = m.strands_info
    return {int(si.rows[si.offsets[s + 1] - 1][1]): int(si.offsets[s + 1] - si.offsets[s]) for s in range(si.n_strands)}


# ---- (1) the reference's own run -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pins():
    assert os.path.exists(_PINS), "tests/golden/ref_growth_pins.npz is part of the repository"
    return np.load(_PINS)


def pin_cases(pins):
    return [str(c) for c in pins["meta_cases"]]


def model_for_pin(pins, case, device="cpu"):
    """This repository's growth model of the pinned case, checked to BE the state the reference was given."""
    tag = str(pins[f"case_{case}_model"])
    seed = int(tag[1:])
    m = growth_model(seed, num_points_strand=int(pins[f"case_{case}_num_points_strand"]), k_avg=int(pins[f"case_{case}_k"]))
    k = f"{tag}_"
    assert np.array_equal(m.endpoint_pairs.numpy(), pins[k + "pairs"])
    for gr in m.optimizer.param_groups:
        assert np.array_equal(gr["params"][0].detach().numpy(), pins[k + gr["name"]]), gr["name"]
    return to_cuda(m) if device != "cpu" else m


def pinned_rows(pins, case):
    k = f"case_{case}_"
    return [pins[k + n] for n in ("pairs", "endpoints", "f_dc", "f_rest", "opacity", "mask", "width")]


def growth_length_of(pins, case):
    gl = float(pins[f"case_{case}_growth_length"])
    return None if np.isnan(gl) else gl


def test_pins_cover_the_contract(pins):
    cases = pin_cases(pins)
    ks = {int(pins[f"case_{c}_k"]) for c in cases}
    gls = {growth_length_of(pins, c) for c in cases}
    grown = [int(pins[f"case_{c}_grow"]) for c in cases]
    assert {1, 3, 5} <= ks and {0.002, None} <= gls and 0 in grown and max(grown) > 0


def test_host_growth_equals_the_reference_run(pins):
    """growing() of the CPU model (the numpy form) appends exactly the rows the reference's growing() passed to cat_segments --
    and the masks it computed and left out -- with the same counter."""
    for case in pin_cases(pins):
        m = model_for_pin(pins, case)
        n0 = m.endpoint_pairs.shape[0]
        info = Info()
        m.growing(info, growth_length=growth_length_of(pins, case))
        want = pinned_rows(pins, case)
        assert info.densification_info["grow"] == int(pins[f"case_{case}_grow"]) == want[0].shape[0], case
        assert info.densification_info["grow_skipped_shared_tip"] == 0
        got = grown_rows(m, n0)
        for name, a, b in zip(("pairs", "endpoints") + GROUPS[1:], got, want):
            assert a.reshape(-1).tobytes() == b.astype(a.dtype).reshape(-1).tobytes() and a.size == b.size, (case, name)


# ---- (2) the loop restatement, with background segments and shared tips --------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("k_avg,growth_length", [(1, 0.002), (3, None), (5, 0.002), (8, None), (12, 0.002), (32, 0.01)])
def test_host_growth_equals_the_loop_restatement(seed, k_avg, growth_length):
    m = growth_model(seed, background=True, k_avg=k_avg)
    want, counter, shared = restated_growth(m, growth_length)
    n0 = m.endpoint_pairs.shape[0]
    before = (m.endpoint_pairs.numpy().copy(), m._endpoints.shape[0], strand_tips(m))
    info = Info()
    m.growing(info, growth_length=growth_length)
    assert info.densification_info == {"grow": counter, "grow_skipped_shared_tip": shared}
    for a, b in zip(grown_rows(m, n0), want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert_consistent_after_growth(m, before, counter)


def test_background_models_have_shared_tips_and_growth():
    got = [restated_growth(growth_model(s, background=True), 0.002)[1:] for s in range(8)]
    assert sum(c for c, _ in got) > 0 and sum(s for _, s in got) > 0


@pytest.mark.parametrize("seed", range(4))
def test_grown_model_is_consistent(seed):
    m = growth_model(seed, num_points_strand=80)
    before = (m.endpoint_pairs.numpy().copy(), m._endpoints.shape[0], strand_tips(m))
    info = Info()
    m.growing(info)
    grown = info.densification_info["grow"]
    assert grown > 0 and m._storage_dirty
    assert_consistent_after_growth(m, before, grown)


def test_nothing_to_grow_is_a_no_op():
    m = growth_model(0, num_points_strand=1)
    tensors = [m.endpoint_pairs] + [getattr(m, a) for _, a in m._PARAM_ATTRS]
    info = Info()
    m.growing(info)
    assert info.densification_info == {"grow": 0, "grow_skipped_shared_tip": 0}
    assert all(a is b for a, b in zip(tensors, [m.endpoint_pairs] + [getattr(m, a) for _, a in m._PARAM_ATTRS]))
    assert not m._storage_dirty


def test_growth_averaging_points_beyond_the_mask_is_refused():
    m = growth_model(0, k_avg=33)
    with pytest.raises(ValueError):
        m.growing(Info())


def test_growth_is_a_scheduled_topology_event():
    """topology_due lists "grow" at multiples of growth_interval: the graphed loop runs that iteration eagerly and re-captures."""
    from train import topology_due
    m = growth_model(0)
    opt = OptimizationParams()
    opt.growth_interval = 5
    assert "grow" in topology_due(m, opt, 10) and "grow" not in topology_due(m, opt, 11)
    assert "grow" not in topology_due(m, OptimizationParams(), 30000)          # (default interval 100000)
