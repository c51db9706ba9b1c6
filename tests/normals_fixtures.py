"""Inputs and host-side restatements for the point-cloud normal tests (tests/test_normals_cpu.py, tests/test_normals_gpu.py).
Everything is generated from seeds; the yardstick is the host path of utils.normals and plain numpy / scipy."""
import numpy as np

TIE_REL = 1e-12          # a point is tied when its K-th and (K+1)-th reference distances are this close (relative)
FRAGILE_REL = 1e-12      # fragile in sign: a non-self neighbour with |proj| <= this * sqrt(largest eigenvalue)
DIRECTION_TOL = 1e-14    # |n_dev x n_host| <= this / g  (g: relative eigen-gap of the reference covariance)
UNIT_TOL = 4 * 2.0 ** -52


def cloud(inp):
    """The named inputs of the tests, float32 [N, 3]."""
    import synthetic
    from tests.synth_fixtures import sphere_mesh
    if inp == "strands-50k":
        return synthetic.strand_polylines(500, 99, seed=0).reshape(-1, 3).astype(np.float32)
    if inp == "strands-200k":
        return synthetic.strand_polylines(2000, 99, seed=1).reshape(-1, 3).astype(np.float32)
    if inp == "cloud":
        return (np.random.default_rng(0).normal(size=(50000, 3)) * 0.1).astype(np.float32)
    if inp == "sphere":
        v = np.asarray(sphere_mesh(0.085, 64, 128)[0], dtype=np.float64)
        return (v + np.random.default_rng(1).normal(size=v.shape) * 1e-4).astype(np.float32)
    if inp == "sheet":
        r = np.random.default_rng(2)
        xy = r.uniform(-1, 1, (20000, 2))
        z = 1e-3 * r.normal(size=20000)
        return np.column_stack([xy, z]).astype(np.float32)
    if inp == "lattice":
        a = np.arange(12)
        return (np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3) * 0.01).astype(np.float32)
    raise KeyError(inp)


FIVE = ("strands-50k", "strands-200k", "cloud", "sphere", "sheet")


def d2_rule1(p, q):
    """Rule 1's expression in float64, operation by operation (numpy does not contract)."""
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def reference(p32, K, chunk=1 << 15):
    """What the comparisons need from the reference side, for float32 (or float64) points and K < N:
    nb [N, K+1] and dist [N, K+1] of cKDTree.query(k=K+1); tied [N]; the host path's normals n_host; per point the relative
    eigen-gap g and the largest eigenvalue l2 of the host-order covariance of the K reference neighbours; fragile [N];
    distinct [N]: no two of the K + 1 smallest rule-1 distances are equal."""
    from scipy.spatial import cKDTree
    from utils.normals import estimate_pointcloud_normals
    p = np.asarray(p32, dtype=np.float64)
    N = p.shape[0]
    dist, nb = cKDTree(p).query(p, k=K + 1, workers=16)
    tied = (dist[:, K] - dist[:, K - 1]) <= TIE_REL * dist[:, K - 1]
    n_host = estimate_pointcloud_normals(p, K)
    g, l2 = np.empty(N), np.empty(N)
    fragile, distinct = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    for s in range(0, N, chunk):
        rows = nb[s:s + chunk, :K]
        knn = p[rows]
        b = knn - knn.mean(axis=1, keepdims=True)
        lam = np.linalg.eigvalsh(np.einsum("cki,ckj->cij", b, b) / K)
        g[s:s + chunk] = (lam[:, 1] - lam[:, 0]) / lam.sum(axis=1)
        l2[s:s + chunk] = lam[:, 2]
        proj = np.einsum("cki,ci->ck", knn - p[s:s + chunk, None, :], n_host[s:s + chunk])
        other = rows != np.arange(s, s + rows.shape[0])[:, None]
        fragile[s:s + chunk] = (other & (np.abs(proj) <= FRAGILE_REL * np.sqrt(lam[:, 2:3]))).any(axis=1)
        d2 = np.sort(d2_rule1(p[s:s + chunk, None, :], p[nb[s:s + chunk]]), axis=1)
        distinct[s:s + chunk] = (np.diff(d2, axis=1) > 0).all(axis=1)
    return dict(p=p, nb=nb, dist=dist, tied=tied, n_host=n_host, g=g, l2=l2, fragile=fragile, distinct=distinct)


def brute_force_rows(p32, K, chunk=512):
    """[N, K] neighbour indices in (rule-1 d2, index) order by a chunked numpy brute force: a stable sort by d2 keeps equal
    distances in ascending index order."""
    p = np.asarray(p32, dtype=np.float64)
    out = np.empty((p.shape[0], K), dtype=np.int64)
    for s in range(0, p.shape[0], chunk):
        d2 = d2_rule1(p[s:s + chunk, None, :], p[None, :, :])
        out[s:s + chunk] = np.argsort(d2, axis=1, kind="stable")[:, :K]
    return out


def host_restatement(p, K):
    """The host algorithm written out again (cKDTree + eigh + vote), for the bit-for-bit check of device=None."""
    from scipy.spatial import cKDTree
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    _, nb = cKDTree(p).query(p, k=K, workers=16)
    knn = p[nb.reshape(p.shape[0], K)]
    b = knn - knn.mean(axis=1, keepdims=True)
    cov = np.einsum("cki,ckj->cij", b, b) / K
    _, vecs = np.linalg.eigh(cov)
    nrm = vecs[:, :, 0]
    proj = np.einsum("cki,ci->ck", knn - p[:, None, :], nrm)
    flip = (proj > 0).sum(axis=1) < 0.5 * K
    return np.where(flip[:, None], -nrm, nrm)
