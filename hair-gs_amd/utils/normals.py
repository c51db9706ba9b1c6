"""Point-cloud normals (pytorch3d.ops.estimate_pointcloud_normals, which the reference's hair and head loaders call; pytorch3d is
not installed here): for every point, its K nearest neighbours (the point itself included) by a cKDTree, the covariance about
their mean, and the eigenvector of its smallest eigenvalue (numpy.linalg.eigh); the sign is flipped when fewer than K / 2
neighbours q have (q - p) . n > 0.  Host only; the result is not pinned to pytorch3d's (an ill-conditioned smallest eigenvector
of a nearly collinear neighbourhood may come out in another direction)."""
import numpy as np

MAX_WORKERS = 16


def estimate_pointcloud_normals(points, neighborhood_size=50, chunk=1 << 16):
    """float64 [N, 3] unit normals of points [N, 3]."""
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
