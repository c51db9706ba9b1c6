"""Point-cloud normals (pytorch3d.ops.estimate_pointcloud_normals, which the reference's hair and head loaders call; pytorch3d is
not installed here).  Two backends follow one contract.

The contract, for points p (float64 [N, 3]; float32 input is widened exactly) and K = min(neighborhood_size, N):

1. Neighbours: the K points with the smallest d2 = (dx*dx + dy*dy) + dz*dz, evaluated in float64 operation by operation (no
   contraction), the point itself included.  Equal d2: the lower index first.  (The host path asks a scipy cKDTree, which does not
   promise an order among exact ties: that is the only place where the host path may choose differently.)
2. Covariance of the neighbours about their mean, divided by K, in float64.
3. Normal: the unit eigenvector of the smallest eigenvalue.
4. Sign: flipped when fewer than K / 2 neighbours q have (q - p) . n > 0.  With K even this makes the result independent of the
   sign the eigen-solver returned: the point itself contributes exactly 0, so a count c under n is K - 1 - c under -n, and exactly
   one of the two is below K / 2.  With K odd the count (K - 1) / 2 maps to itself and the sign is the solver's; the tests
   compare signs for even K only.

Covariances whose two smallest eigenvalues coincide exactly (N = 1, K <= 2, all neighbours collinear or identical) have no defined
normal: the output is finite and of unit length, nothing more.

Host path (device=None or "cpu", the default everywhere): cKDTree, numpy.linalg.eigh.  Device path (device="cuda";
csrc/hgs_normals.hip): a grid search with one wavefront per point, K <= DEVICE_MAX_NEIGHBORS; its result depends only on each
point's neighbour set and the neighbours' ranks in (d2, index) order, so it is bitwise reproducible and equivariant under a
permutation of the input wherever the K + 1 smallest distances of a point are distinct.  Neither result is pinned to pytorch3d's
(an ill-conditioned smallest eigenvector of a nearly collinear neighbourhood may come out in another direction)."""
import numpy as np

MAX_WORKERS = 16
DEVICE_MAX_NEIGHBORS = 64


def _check_device_args(shape, neighborhood_size):
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"point-cloud normals take points of shape [N, 3], got {tuple(shape)}")
    if int(neighborhood_size) < 1:
        raise ValueError(f"neighborhood_size = {neighborhood_size} must be at least 1")
    if min(int(neighborhood_size), shape[0]) > DEVICE_MAX_NEIGHBORS:
        raise ValueError(f"neighborhood_size = {neighborhood_size}: the device path holds at most {DEVICE_MAX_NEIGHBORS} "
                         "neighbours (one per lane of a wavefront); use the host path")


def estimate_pointcloud_normals_device(points, neighborhood_size=50, return_neighbors=False):
    """Batched device form: points = float64 (or float32, widened) tensor [N, 3] on a CUDA(HIP) device -> float64 normals [N, 3]
    on that device (+ the int32 neighbour indices [N, K] in rank order with return_neighbors).  Raises before any launch:
    TypeError for anything but such a tensor, ValueError for another shape, K > DEVICE_MAX_NEIGHBORS or non-finite coordinates."""
    import torch
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise TypeError("estimate_pointcloud_normals_device takes a float64 or float32 tensor [N, 3]")
    _check_device_args(points.shape, neighborhood_size)
    if not points.is_cuda:
        raise TypeError("estimate_pointcloud_normals_device takes a tensor on the GPU (the host path: estimate_pointcloud_normals)")
    import hgs_runtime as rt
    p = rt.require_gpu_tensor(points.to(torch.float64).contiguous(), "points", torch.float64)
    N = p.shape[0]
    K = min(int(neighborhood_size), N)
    dev = p.device
    normals = torch.empty((N, 3), dtype=torch.float64, device=dev)
    nb = torch.empty((N, K), dtype=torch.int32, device=dev) if return_neighbors else None
    if N > 0:
        if not bool(torch.isfinite(p).all()):          # a NaN must never reach the grid walk
            raise ValueError("point-cloud normals need finite coordinates")
        L = rt.lib()
        scratch = torch.empty(int(L.hgs_pointcloud_normals_scratch_bytes(N, K)), dtype=torch.uint8, device=dev)
        rt.check(L.hgs_pointcloud_normals(rt.current_stream(), N, K, rt.ptr(p), rt.ptr(normals), rt.ptr(nb), rt.ptr(scratch),
                                          scratch.numel()))
    return (normals, nb) if return_neighbors else normals


def estimate_pointcloud_normals(points, neighborhood_size=50, chunk=1 << 16, device=None):
    """float64 [N, 3] unit normals of points [N, 3] (module docstring: the contract).  device=None or "cpu": the host path;
    device="cuda": the HIP kernels (host array in, host array out)."""
    if device is not None and str(device) != "cpu":
        p = np.asarray(points)
        if p.dtype != np.float32:
            p = p.astype(np.float64, copy=False)
        _check_device_args(p.shape, neighborhood_size)
        if not np.isfinite(p).all():
            raise ValueError("point-cloud normals need finite coordinates")
        if p.shape[0] == 0:
            return np.zeros((0, 3))
        import torch
        t = torch.from_numpy(np.ascontiguousarray(p)).to(device)
        return estimate_pointcloud_normals_device(t, neighborhood_size).cpu().numpy()
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, 3))
    K = min(int(neighborhood_size), n)
    tree = cKDTree(p)
    out = np.empty((n, 3))
    for s in range(0, n, chunk):
        q = p[s:s + chunk]
        _, nb = tree.query(q, k=K, workers=MAX_WORKERS)
        nb = nb.reshape(q.shape[0], K)
        knn = p[nb]                                             # [c, K, 3]
        b = knn - knn.mean(axis=1, keepdims=True)
        cov = np.einsum("cki,ckj->cij", b, b) / K
        _, vecs = np.linalg.eigh(cov)
        nrm = vecs[:, :, 0]
        proj = np.einsum("cki,ci->ck", knn - q[:, None, :], nrm)
        flip = (proj > 0).sum(axis=1) < 0.5 * K
        out[s:s + chunk] = np.where(flip[:, None], -nrm, nrm)
    return out
