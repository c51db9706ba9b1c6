"""Float64 reference of the magnet term, the fp32 yardstick and the comparator built on them (tests/test_magnet_f64_cpu.py,
tests/test_magnet_gpu.py).

`loop_reference` restates loss/losses.py strand_joints_magnet_loss (:124-164) as loops over the ends, in the dtype it is given:
float64 is the reference, float32 carries the mutants the comparator has to reject.  It returns what the statement never
exposes -- the selection and the masks -- next to the value and the gradient, which it forms from the selection by the closed
form (include/hgs.h (g)): 4 s (p - q) / m to the end, the opposite to its neighbour.  `torch_statement` is the statement
itself, line for line, with those intermediates returned; the CPU test ties it to strand_joints_magnet_loss bit for bit, so
the yardstick is the project's own fp32 arithmetic.

The comparator follows tests/param_reference.py (the project's rule for "no worse than an fp32 restatement"): per case
max|x - x64| <= K max(e_ref, 4 ulp scale) with e_ref = max|x32 - x64| the fp32 statement's own error and K = 8; selection and
row count must be equal."""
import types

import numpy as np
import torch

from tests import param_reference as R

K = 8.0              # tests/test_params_f64_cpu.py K_MAX, tests/test_params_f64_gpu.py K
MUTANTS = ("square", "no_neighbour_grad", "tie_larger", "ranks_not_compacted", "partner_by_position")


def model_of(pts, device="cpu"):
    from scene.hair_gaussian_model import HairGaussianModel
    return HairGaussianModel.from_strands(pts, device=device)


def level_edge_model(pts, n, device="cpu"):
    """The model of tests/magnet_cases.level_edge(family, n) with exactly n ends.  For an odd n the last segment of the last
    strand is re-attached to endpoint 1 (the middle vertex of strand 0, then of degree 3): the last strand's tip is in no
    segment any more, and the list of ends is the first n of the family's n + 1 points.  The degree-3 vertex is deliberate and
    inert: the term reads the degree-1 endpoints and each one's segment partner, nothing else of the topology, and a set of
    chains cannot have an odd number of ends.  (Collapsing an end segment instead would leave n + 1 ends in the table, and the
    grid's level is chosen from the table's size: 1023 would run at the level of 1024.)"""
    m = model_of(pts, device)
    if n % 2:
        m.endpoint_pairs[-1, 1] = 1
    return m


def topology(model):
    """(ends, partner, mapping) as the statement builds them (:134-138), numpy int64."""
    E = model._endpoints.shape[0]
    if model.endpoint_pairs.numel() == 0:          # (a model without segments: the helpers below take max() of the table)
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(E, dtype=np.int64)
    u, c = torch.unique(model.endpoint_pairs, return_counts=True)
    ends = u[c == 1]
    comp, _ = model.get_complementary_endpoint_idx(ends)
    mapping = torch.zeros(E, dtype=torch.long, device=ends.device)
    mapping[ends] = comp
    return ends.cpu().numpy(), comp.cpu().numpy(), mapping.cpu().numpy()


def _norm(v):
    return np.sqrt((v * v).sum(dtype=v.dtype))


def loop_reference(endpoints, ends, partner, mapping, min_val, dtype=np.float64, mutant=None):
    """endpoints [E,3] (float32 values), the topology of topology().  Returns a namespace: value, grad [E,3], nv (valid ends),
    rows (rows of the mean), sel [nv] (selected position, -1 where the row is not kept), nn [nv,3] / d2 [nv,3] (the three
    nearest by (distance, position), -1 / inf where missing), valid [n], found / second_ok / nn_mask / final [nv]."""
    assert mutant is None or mutant in MUTANTS
    with np.errstate(all="ignore"):
        ep = np.asarray(endpoints).astype(dtype)
        n, E = len(ends), ep.shape[0]
        mv = dtype(min_val)
        valid = np.zeros(n, dtype=bool)
        for i in range(n):
            valid[i] = _norm(ep[ends[i]] - ep[partner[i]]) > mv                      # (a)
        keep = np.ones(n, dtype=bool) if mutant == "ranks_not_compacted" else valid
        cends, cpart = ends[keep], partner[keep]
        listed = valid[keep]                                                         # (all True unless the mutant is on)
        pts = ep[cends]
        nv = len(cends)
        nn = np.full((nv, 3), -1, dtype=np.int64)
        d2 = np.full((nv, 3), np.inf, dtype=dtype)
        sel = np.full(nv, -1, dtype=np.int64)
        sq = np.zeros(nv, dtype=dtype)
        found, second_ok, nn_mask, final = (np.zeros(nv, dtype=bool) for _ in range(4))
        if nv >= 3:
            pos_of = {int(g): k for k, g in enumerate(cends)}
            for a in range(nv):
                diff = pts[a][None, :] - pts
                dist = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]
                comparable = np.nonzero(dist < np.inf)[0]                            # (b): NaN and inf compare closer to nothing
                prefer = -comparable if mutant == "tie_larger" else comparable
                order = comparable[np.lexsort((prefer, dist[comparable]))][:3]
                nn[a, :len(order)] = order
                d2[a, :len(order)] = dist[order]
                found[a] = len(order) == 3                                           # (e)
                n1, n2 = max(nn[a, 1], 0), max(nn[a, 2], 0)
                other = pos_of.get(int(cpart[a]), -2) if mutant == "partner_by_position" else cpart[a]
                second_ok[a] = n1 != a and n1 != other                               # (c)
                q = n1 if second_ok[a] else n2
                s = d2[a, 1] if second_ok[a] else d2[a, 2]
                nn_mask[a] = _norm(ep[q] - ep[mapping[q]]) > mv                      # (d): the position as a global id
                final[a] = listed[a] and nn_mask[a] and found[a] and np.isfinite(s)
                if final[a]:
                    sel[a], sq[a] = q, s
        rows = int(final.sum())
        grad = np.zeros((E, 3), dtype=dtype)
        value = dtype(0.0)
        if rows > 0:
            terms = sq[final] if mutant == "square" else sq[final] * sq[final]
            value = terms.sum(dtype=dtype) / dtype(rows)                             # (f)
            for a in np.nonzero(final)[0]:
                q = sel[a]
                g = (dtype(2.0) if mutant == "square" else dtype(4.0) * sq[a]) * (pts[a] - pts[q]) / dtype(rows)    # (g)
                grad[cends[a]] += g
                if mutant != "no_neighbour_grad":
                    grad[cends[q]] -= g
    return types.SimpleNamespace(value=value, grad=grad, nv=nv, rows=rows, sel=sel, nn=nn, d2=d2, valid=valid, found=found,
                                 second_ok=second_ok, nn_mask=nn_mask, final=final)


def torch_statement(gaussians, knn=None):
    """loss/losses.py:124-164 line for line, returning (loss, namespace of the intermediates: nv, sel, final, second_ok,
    nn_mask, valid).  `knn`: the neighbour search (default: loss.losses.knn3_self, as the statement)."""
    from loss.losses import knn3_self
    knn = knn3_self if knn is None else knn
    ep = gaussians._endpoints
    u, c = torch.unique(gaussians.endpoint_pairs, return_counts=True)
    ends = u[c == 1]
    comp, _ = gaussians.get_complementary_endpoint_idx(ends)
    mapping = torch.zeros(ep.shape[0], device=ep.device, dtype=torch.long)
    mapping[ends] = comp
    det = ep.detach()
    self_dir = det[ends] - det[comp]
    valid = torch.norm(self_dir, dim=1) > gaussians.min_val
    valid_all = valid
    self_dir, ends, comp = self_dir[valid], ends[valid], comp[valid]
    pts = ep[ends]
    n = pts.shape[0]
    info = types.SimpleNamespace(nv=n, valid=valid_all.cpu().numpy(), sel=np.full(n, -1, dtype=np.int64), rows=0,
                                 final=np.zeros(n, dtype=bool), second_ok=np.zeros(n, dtype=bool), nn_mask=np.zeros(n, dtype=bool))
    if n < 3:
        return pts.sum() * 0.0, info
    _, nn = knn(pts)
    found = (nn >= 0).all(dim=1)
    nn = nn.clamp(min=0)
    sq = ((pts[:, None, :] - pts[nn]) ** 2).sum(dim=-1)
    self_idx = torch.arange(n, device=ep.device)
    second_ok = (nn[:, 1] != self_idx) & (nn[:, 1] != comp)
    sq = torch.where(second_ok, sq[:, 1], sq[:, 2])
    nn = torch.where(second_ok, nn[:, 1], nn[:, 2])
    self_mask = torch.norm(self_dir, dim=1, keepdim=True) > gaussians.min_val
    nn_dir = det[nn] - det[mapping[nn]]
    nn_mask = torch.norm(nn_dir, dim=1, keepdim=True) > gaussians.min_val
    final = (self_mask & nn_mask).reshape(-1) & found & torch.isfinite(sq.detach())
    info.final, info.second_ok, info.nn_mask = final.cpu().numpy(), second_ok.cpu().numpy(), nn_mask.reshape(-1).cpu().numpy()
    info.sel = torch.where(final, nn, torch.full_like(nn, -1)).cpu().numpy()
    info.rows = int(final.sum())
    sq = sq[final]
    if sq.numel() == 0:
        return pts.sum() * 0.0, info
    return torch.mean(sq * sq), info


def reference(pts, min_val=None):
    """The float64 loop reference and the fp32 torch statement (value, gradient, intermediates) of a case on a CPU model."""
    m = model_of(pts, "cpu")
    mv = float(m.min_val if min_val is None else min_val)
    ends, partner, mapping = topology(m)
    r64 = loop_reference(pts.reshape(-1, 3), ends, partner, mapping, mv)
    if len(ends) == 0:
        # a model without segments: get_complementary_endpoint_idx cannot run on an empty table, so the statement has no fp32
        # value of its own; by its n < 3 rule the term is exactly 0 and so is the yardstick
        r32 = loop_reference(pts.reshape(-1, 3), ends, partner, mapping, mv, dtype=np.float32)
        r32.nan_rows = np.zeros(0, dtype=np.int64)
        return types.SimpleNamespace(r64=r64, r32=r32, ends=ends, partner=partner, mapping=mapping, min_val=mv,
                                     E=pts.reshape(-1, 3).shape[0])
    loss, info = torch_statement(m)
    m._endpoints.grad = None
    loss.backward()
    r32 = info
    r32.value = np.float32(loss.detach().numpy())
    g32 = m._endpoints.grad.numpy().copy()
    # An end with an infinite coordinate stays in the list; the statement masks its row out of the mean, but autograd's backward
    # of the square still multiplies the row's zero gradient with the infinite difference: NaN at that end and at the ends its
    # neighbour slots point to.  Float64 (and the device op) give exactly 0 there -- rows left out contribute nothing.  Such
    # endpoints are reported in nan_rows and carry no fp32 error of their own: the allowance comes from the finite ones.
    r32.nan_rows = np.nonzero(~np.isfinite(g32).all(axis=1))[0]
    g32[r32.nan_rows] = r64.grad[r32.nan_rows].astype(np.float32)
    r32.grad = g32
    return types.SimpleNamespace(r64=r64, r32=r32, ends=ends, partner=partner, mapping=mapping, min_val=mv, E=pts.reshape(-1, 3).shape[0])


def ratios(value, grad, ref):
    """(value ratio, gradient ratio) of a candidate against ref.r64 with ref.r32's own error as the allowance
    (param_reference.class_ratios: max|x - x64| / max(e_ref, 4 ulp scale); where float64 is exactly 0 the candidate must be)."""
    one = np.array(["*"])
    rv = R.worst(R.class_ratios(np.array([[value]]), np.array([[ref.r64.value]]), np.array([[ref.r32.value]]), one))
    E = ref.E
    if E == 0:
        return rv, 0.0
    lab = np.array(["*"] * E)
    rg = R.worst(R.class_ratios(np.asarray(grad).reshape(E, 3), ref.r64.grad, ref.r32.grad, lab))
    return rv, rg


def accepts(value, grad, sel, rows, ref):
    """The comparator: selection and row count equal, value and gradient within K of float64."""
    if int(rows) != ref.r64.rows or not np.array_equal(np.asarray(sel, dtype=np.int64), ref.r64.sel):
        return False
    rv, rg = ratios(value, grad, ref)
    return rv <= K and rg <= K
