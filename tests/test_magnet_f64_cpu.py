"""The magnet term against float64, on the CPU: the float64 loop reference of tests/magnet_reference.py, the fp32 torch
statement (loss/losses.py strand_joints_magnet_loss) as the yardstick, and the comparator tests/test_magnet_gpu.py holds the
device op (include/hgs.h hgs_magnet_*) to.  No case of tests/magnet_cases.py is exempted from any condition.

Measured here (pytest -s prints the table): over the cases the fp32 statement's own value error is at most 0.42 of the floor
(4 ulp of the value) and its gradient error at most 0.32 of max(e_ref, 4 ulp of the largest gradient) -- by construction the
statement sits at ratio <= 1 of its own allowance; the margin K = 8 is tests/param_reference.py's."""
import os
import re

import numpy as np
import pytest
import torch

from tests import magnet_cases as MC
from tests import magnet_reference as MR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = MR.reference(MC.cases()[name])
    return _REF[name]


def test_case_list_covers_what_the_term_can_meet():
    ends = {k: len(_ref(k).ends) for k in MC.NAMES}
    assert (ends["no_strands"], ends["one_strand"], ends["two_strands"]) == (0, 2, 4)
    assert list(_ref("one_segment_3").ends) == [0, 1, 2, 3, 4, 5]                 # one-segment strands: ids == positions
    assert list(_ref("multi_segment").ends[:4]) == [0, 12, 13, 25]                # multi-segment strands: they differ
    assert [_ref(f"valid_{k}").r64.nv for k in (255, 256, 257)] == [255, 256, 257]
    for k, first_invalid in (("collapsed_first", 0), ("collapsed_last", 59)):
        assert list(np.nonzero(~_ref(k).r64.valid)[0]) == [first_invalid]
    assert 0 < np.nonzero(~_ref("collapsed_middle").r64.valid)[0].min() and _ref("collapsed_middle").r64.nv == 58
    # the quirks are exercised: (c) takes the third neighbour, (d) drops rows, non-finite ends drop rows
    assert (~_ref("one_segment_40").r64.second_ok).sum() > 10 and (~_ref("multi_segment").r64.second_ok).sum() == 0
    assert (~_ref("short_lookup").r64.nn_mask).sum() >= 2
    hit = _ref("partner_id_hit").r64
    assert list(np.nonzero(~hit.second_ok)[0]) == [0] and hit.nn[0, 1] == 1 and _ref("partner_id_hit").partner[0] == 1
    r = _ref("nonfinite").r64
    assert r.nv == 59 and (~r.found).sum() == 1 and r.rows < r.nv
    assert _ref("coincident").r64.rows == 24 and _ref("coincident").r64.value == 0.0
    lat = _ref("lattice").r64
    assert (lat.d2[:, 1] == lat.d2[:, 2]).sum() > 10                               # real ties in the lattice
    assert _ref("one_strand").r64.rows == 0 and _ref("no_strands").r64.rows == 0   # the n < 3 rules


@pytest.mark.parametrize("n", MC.LEVEL_EDGE_SIZES)
@pytest.mark.parametrize("family", MC.LEVEL_EDGE_FAMILIES)
def test_level_edge_inputs_have_n_valid_ends(family, n):
    """The inputs of tests/test_magnet_gpu.py::test_grid_path_where_its_level_changes really straddle the level edges: the
    table holds exactly n ends (the grid's level is chosen from that number) and at least n - 1 of them are valid."""
    m = MR.level_edge_model(MC.level_edge(family, n), n)
    ends, partner, _ = MR.topology(m)
    ep = m._endpoints.detach()
    valid = torch.norm(ep[ends] - ep[partner], dim=1) > m.min_val
    assert len(ends) == n and int(valid.sum()) >= n - 1
    assert np.isfinite(ep.numpy()).all()


@pytest.mark.parametrize("name", MC.NAMES)
def test_fp32_statement_is_the_projects_and_selects_like_float64(name):
    """tests/magnet_reference.torch_statement IS strand_joints_magnet_loss (same bits), and in float32 it selects the same
    neighbours and masks as the float64 loops; the comparator passes it."""
    from loss.losses import strand_joints_magnet_loss
    ref = _ref(name)
    if len(ref.ends):
        m = MR.model_of(MC.cases()[name])
        loss = strand_joints_magnet_loss(m)
        loss.backward()
        g = m._endpoints.grad.numpy()
        assert np.float32(loss.detach().numpy()).tobytes() == ref.r32.value.tobytes()
        keep = np.ones(ref.E, dtype=bool)
        keep[ref.r32.nan_rows] = False
        assert g[keep].tobytes() == ref.r32.grad[keep].tobytes() and not np.isfinite(g[~keep]).all(axis=1).any()
    r32, r64 = ref.r32, ref.r64
    assert r32.nv == r64.nv and r32.rows == r64.rows
    for k in ("valid", "sel", "final", "second_ok", "nn_mask"):
        if k in ("second_ok", "nn_mask"):       # (only meaningful on rows with three neighbours)
            np.testing.assert_array_equal(getattr(r32, k)[r64.found], getattr(r64, k)[r64.found], err_msg=k)
        else:
            np.testing.assert_array_equal(getattr(r32, k), getattr(r64, k), err_msg=k)
    # autograd's 0 x inf: only in the case with an infinite end, only at that end and where its neighbour slots point
    if name == "nonfinite":
        inf_end = int(np.nonzero(np.isinf(MC.cases()[name].reshape(-1, 3)).any(axis=1))[0][0])
        assert inf_end in r32.nan_rows and len(r32.nan_rows) <= 4
    else:
        assert len(r32.nan_rows) == 0
    rv, rg = MR.ratios(r32.value, r32.grad, ref)
    print(f"ratio | fp32 statement | {name} | value {rv:.2f} | gradient {rg:.2f} |")
    assert MR.accepts(r32.value, r32.grad, r32.sel, r32.rows, ref)


@pytest.mark.parametrize("mutant,name", [("square", "multi_segment"), ("no_neighbour_grad", "multi_segment"),
                                         ("tie_larger", "lattice"), ("ranks_not_compacted", "collapsed_first"),
                                         ("partner_by_position", "partner_id_hit"), ("partner_by_position", "coincident")])
def test_comparator_rejects_mutants(mutant, name):
    ref = _ref(name)
    pts = MC.cases()[name].reshape(-1, 3)
    good = MR.loop_reference(pts, ref.ends, ref.partner, ref.mapping, ref.min_val, dtype=np.float32)
    assert MR.accepts(good.value, good.grad, good.sel, good.rows, ref)           # the fp32 loops themselves pass
    bad = MR.loop_reference(pts, ref.ends, ref.partner, ref.mapping, ref.min_val, dtype=np.float32, mutant=mutant)
    assert not MR.accepts(bad.value, bad.grad, bad.sel, bad.rows, ref)


def test_partner_by_position_is_invisible_where_ids_are_positions():
    """One-segment strands: the global ids equal the positions, so the statement's comparison with the GLOBAL id does exclude the
    partner there -- the quirk shows only on multi-segment strands (the mutant above)."""
    ref = _ref("one_segment_40")
    pts = MC.cases()["one_segment_40"].reshape(-1, 3)
    bad = MR.loop_reference(pts, ref.ends, ref.partner, ref.mapping, ref.min_val, dtype=np.float32, mutant="partner_by_position")
    assert MR.accepts(bad.value, bad.grad, bad.sel, bad.rows, ref)


def test_library_exports_the_magnet_entry_points():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    src = open(os.path.join(ROOT, "include", "hgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hgs_[a-z0-9_]*magnet[a-z0-9_]*)\s*\(", src))
    assert declared == {"hgs_magnet_scratch_bytes", "hgs_magnet_forward", "hgs_magnet_backward", "hgs_set_magnet_search"}
    for name in declared:
        assert name in rt.SIGNATURES and hasattr(L, name), name
    # sizes: monotone in n, room for the padded sort keys, and nothing for nonsense
    b = [L.hgs_magnet_scratch_bytes(n, 2 * n) for n in (0, 1, 255, 256, 257, 2000, 20000, 200000)]
    assert all(x % 256 == 0 for x in b) and b == sorted(b) and b[-1] >= 8 * 262144 and L.hgs_magnet_scratch_bytes(-1, 4) == 0
    was = L.hgs_set_magnet_search(1)             # (process-wide: whatever an earlier test left is put back)
    try:
        assert was in (-1, 0, 1) and L.hgs_set_magnet_search(0) == 1 and L.hgs_set_magnet_search(-1) == 0
        assert L.hgs_set_magnet_search(7) == -1 and L.hgs_set_magnet_search(-5) == 1     # (non-zero: grid, negative: automatic)
    finally:
        L.hgs_set_magnet_search(was)


def test_fused_magnet_is_off_by_default_and_a_flag():
    from argparse import ArgumentParser
    from arguments import OptimizationParams
    assert OptimizationParams().fused_magnet is False
    parser = ArgumentParser()
    op = OptimizationParams(parser)
    assert op.extract(parser.parse_args(["--fused_magnet", "--lambda_magnet", "0.1"])).fused_magnet is True
    assert op.extract(parser.parse_args([])).fused_magnet is False
