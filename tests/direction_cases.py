"""Volumes, segments and topologies of the 3-D direction term's tests (tests/test_direction_cpu.py, tests/test_direction_gpu.py): the
smallest at which the kernels of csrc/hgs_direction.hip can go wrong.  A case is (volume name, points f32 [E, 3], pairs int64 [S, 2],
min_conf)."""
import functools

import numpy as np

from utils.direction_term import DirectionVolume
from utils.trace import Field

MIN_CONF = 0.5
BELOW = float(np.nextafter(np.float32(MIN_CONF), np.float32(0)))           # one float32 step below the gate


def _unit(d):
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- volumes ---------------------------------------------------------------------------------------------------------------
def vol2():
    """2 x 2 x 2: one cell, eight distinct lines, confidences around the gate."""
    rng = np.random.default_rng(2)
    d = _unit(rng.normal(size=(2, 2, 2, 3)))
    conf = np.array([0.2, 0.9, 0.6, 1.4, 0.3, 0.8, 1.1, 0.5]).reshape(2, 2, 2)
    return DirectionVolume(Field(np.array([0.1, -0.2, 0.3]), 0.37, (2, 2, 2), d, conf))


def vol543():
    """nx, ny, nz = 5, 4, 3 with a distinct line and confidence at every node, odd origin and spacing: a swapped axis shows."""
    rng = np.random.default_rng(543)
    d = _unit(rng.normal(size=(3, 4, 5, 3)))
    conf = 0.3 + 0.02 * np.arange(60, dtype=np.float64).reshape(3, 4, 5)
    return DirectionVolume(Field(np.array([0.137, -2.411, 1.003]), 0.0731, (5, 4, 3), d, conf))


def swirl33():
    """33^3 nodes over [-1, 1]^3 (h = 1/16: exact in float32): line ~ (-y, x, -0.5) with a random sign per node, conf falling from 2
    to 0 across the shell 0.25 <= r <= 1."""
    rng = np.random.default_rng(33)
    ax = -1.0 + np.arange(33) / 16.0
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    d = _unit(np.stack([-y, x, np.full_like(x, -0.5)], axis=-1))
    d = d * rng.choice([-1.0, 1.0], size=x.shape)[..., None]
    r = np.sqrt(x * x + y * y + z * z)
    conf = 2.0 * np.clip((1.0 - r) / 0.75, 0.0, 1.0)
    return DirectionVolume(Field(np.array([-1.0, -1.0, -1.0]), 0.0625, (33, 33, 33), d, conf))


def constant(direction=(0.0, 0.0, 1.0), n=9, conf=1.0, flip_seed=None):
    """n^3 nodes over [0, 1]^3 holding one line (the behaviour test, gradcheck); flip_seed: a random sign per node."""
    d = np.broadcast_to(_unit(np.asarray(direction, np.float64)), (n, n, n, 3)).copy()
    if flip_seed is not None:
        d = d * np.random.default_rng(flip_seed).choice([-1.0, 1.0], size=(n, n, n))[..., None]
    return DirectionVolume(Field(np.zeros(3), 1.0 / (n - 1), (n, n, n), d, np.full((n, n, n), float(conf))))


def hand7():
    """7^3 nodes over [0, 0.75]^3 (h = 1/8, origin 0: exact in float32), the line (0, 0, 1) with conf 1 everywhere but:
      cell (0, 0, 0): lines (1, 0, 0) on its x = 0 face and (-1, 0, 0) on its x = 1 face (they cancel for a segment along z)
      node (2, 0, 0): line (1, 0, 0) (exactly perpendicular to a segment along z)
      node (4, 2, 0): conf exactly MIN_CONF;  node (4, 4, 0): conf one float32 step below;  node (6, 6, 6): a NaN line, conf -1."""
    d = np.zeros((7, 7, 7, 3))
    d[..., 2] = 1.0
    conf = np.ones((7, 7, 7))
    d[0:2, 0:2, 0] = (1.0, 0.0, 0.0)                 # [iz, iy, ix]
    d[0:2, 0:2, 1] = (-1.0, 0.0, 0.0)
    d[0, 0, 2] = (1.0, 0.0, 0.0)
    conf[0, 2, 4] = MIN_CONF
    conf[0, 4, 4] = BELOW
    d[6, 6, 6] = np.nan
    conf[5, 6, 6] = -1.0
    return DirectionVolume(Field(np.zeros(3), 0.125, (7, 7, 7), d, conf))


VOLUMES = {"vol2": vol2, "vol543": vol543, "swirl33": swirl33, "hand7": hand7, "const9": constant}


@functools.lru_cache(maxsize=None)
def volume(name):
    return VOLUMES[name]()


# ---- segments --------------------------------------------------------------------------------------------------------------
def chains(vol, S, seed, per=7, step=0.6, spill=0.15):
    """S segments as polylines of up to `per` segments: joints walk `step` spacings a time from a start inside the box widened by
    `spill` of its size, so some strands leave it.  Every second strand is listed tip-first."""
    rng = np.random.default_rng(seed)
    lo = vol.origin
    span = (np.array(vol.shape) - 1) * vol.spacing
    pts, pairs, k = [], [], 0
    while len(pairs) < S:
        n = min(per, S - len(pairs))
        x = lo - spill * span + rng.random(3) * (1 + 2 * spill) * span
        walk = x + np.cumsum(np.concatenate([np.zeros((1, 3)), _unit(rng.normal(size=(n, 3))) * step * vol.spacing * rng.uniform(0.3, 1.5, (n, 1))]), axis=0)
        base = len(pts)
        pts.extend(walk)
        for j in range(n):
            pairs.append((base + j + 1, base + j) if k % 2 else (base + j, base + j + 1))
        k += 1
    return np.asarray(pts, np.float64).reshape(-1, 3).astype(np.float32), np.asarray(pairs, np.int64).reshape(-1, 2)


HAND_ROWS = ("zero_length", "same_endpoint", "on_a_node", "last_cell", "t_equals_top", "below_zero", "nan_endpoint", "inf_endpoint",
             "w_below_gate", "w_at_gate", "cancel", "perpendicular_corner", "parallel", "parallel_odd", "perpendicular",
             "cleared_node", "chain_0", "chain_1", "chain_2", "junction_0", "junction_1", "junction_2", "tip_first")
HAND_INACTIVE = ("zero_length", "same_endpoint", "t_equals_top", "below_zero", "nan_endpoint", "inf_endpoint", "w_below_gate", "cancel")


def hand_segments():
    """(points f32 [E, 3], pairs [S, 2]) on hand7, rows named by HAND_ROWS.  Endpoint 0 is used by no segment."""
    pts, pairs = [(0.3, 0.3, 0.3)], []

    def seg(a, b):
        pts.extend([a, b])
        pairs.append((len(pts) - 2, len(pts) - 1))
    seg((0.3, 0.4, 0.5), (0.3, 0.4, 0.5))                                     # zero length: two endpoints at one place
    pts.append((0.4, 0.4, 0.4))
    pairs.append((len(pts) - 1, len(pts) - 1))                                # pairs[s][0] == pairs[s][1]
    seg((0.5, 0.25, 0.375 - 0.0625), (0.5, 0.25, 0.375 + 0.0625))             # midpoint exactly on node (4, 2, 3)
    seg((0.7, 0.7, 0.65), (0.7, 0.71, 0.73))                                  # the last cell (5, 5, 5)
    seg((0.75 - 0.0625, 0.3, 0.3), (0.75 + 0.0625, 0.3, 0.3))                 # t = n - 1 exactly on x: out
    seg((-0.05, 0.3, 0.3), (0.03, 0.3, 0.3))                                  # midpoint below 0
    seg((np.nan, 0.3, 0.3), (0.3, 0.3, 0.3))
    seg((0.3, 0.3, 0.3), (0.3, np.inf, 0.3))
    seg((0.5, 0.5, -0.0625), (0.5, 0.5, 0.0625))                              # on node (4, 4, 0): w = BELOW
    seg((0.5, 0.25, -0.0625), (0.5, 0.25, 0.0625))                            # on node (4, 2, 0): w = MIN_CONF exactly
    seg((0.0625, 0.0625, 0.0), (0.0625, 0.0625, 0.125))                       # centre of cell (0, 0, 0): the corners cancel to v = 0
    seg((0.3125, 0.0625, 0.0), (0.3125, 0.0625, 0.125))                       # centre of cell (2, 0, 0): one corner's dot(c, u) == 0
    seg((0.3, 0.55, 0.375), (0.3, 0.55, 0.625))                               # parallel, u_z = 0.25: term exactly 0
    seg((0.3, 0.55, 0.3), (0.3, 0.55, 0.5))                                   # parallel, u_z not a power of two
    seg((0.25, 0.55, 0.45), (0.5, 0.55, 0.45))                                # perpendicular: term exactly 1
    seg((0.65, 0.65, 0.60), (0.67, 0.67, 0.72))                               # a cell with the cleared nodes (6, 6, 5) and (6, 6, 6)
    base = len(pts)                                                           # a chain of three: two ends, two inner joints
    pts.extend([(0.2, 0.2, 0.30), (0.22, 0.21, 0.38), (0.25, 0.2, 0.46), (0.26, 0.23, 0.55)])
    pairs.extend([(base, base + 1), (base + 1, base + 2), (base + 2, base + 3)])
    base = len(pts)                                                           # a junction: three segments share endpoint `base`
    pts.extend([(0.45, 0.45, 0.45), (0.5, 0.47, 0.52), (0.41, 0.5, 0.5), (0.45, 0.4, 0.36)])
    pairs.extend([(base, base + 1), (base + 2, base), (base, base + 3)])
    pairs.append((base + 3, base + 1))                                        # tip-first, between two used endpoints
    assert len(pairs) == len(HAND_ROWS)
    return np.asarray(pts, np.float64).astype(np.float32), np.asarray(pairs, np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (volume name, points, pairs, min_conf)."""
    out = {}
    for S in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        out[f"swirl_S{S}"] = ("swirl33", *chains(volume("swirl33"), S, 100 + S), MIN_CONF)
    out["swirl_S16641"] = ("swirl33", *chains(volume("swirl33"), 16641, 7), MIN_CONF)      # 66 blocks: the reduction's strided loop
    out["vol2_S65"] = ("vol2", *chains(volume("vol2"), 65, 2, per=3, step=0.2, spill=0.3), MIN_CONF)
    out["vol543_S257"] = ("vol543", *chains(volume("vol543"), 257, 3, per=5, step=0.5), 0.45)
    out["hand"] = ("hand7", *hand_segments(), MIN_CONF)
    out["no_segments"] = ("swirl33", np.zeros((5, 3), np.float32), np.zeros((0, 2), np.int64), MIN_CONF)   # E > 0, S = 0
    return out


NAMES = ("swirl_S0", "swirl_S1", "swirl_S63", "swirl_S64", "swirl_S65", "swirl_S255", "swirl_S256", "swirl_S257", "swirl_S513",
         "swirl_S16641", "vol2_S65", "vol543_S257", "hand", "no_segments")
RANDOM = tuple(n for n in NAMES if n.startswith("swirl_S"))


def case(name):
    vol, pts, pairs, min_conf = cases()[name]
    return volume(vol), pts, pairs, min_conf
