"""The rescaling contract restated term by term in plain Python floats (float64, one rounding per operation), independent of
hair-gs_amd/utils/rescale.py: the footprint and its weights, the image and mask sums, and the double-angle average of an orientation
pair, whose angle byte is found by counting the boundaries one at a time.  Meant for the small sizes of tests/test_rescale_cpu.py."""
import math

import numpy as np


def taps(x, S, D):
    """[(source index, weight)] of output index x along an axis of S source and D output pixels, every tap of the contract."""
    lo = float(x * S) / float(D)
    hi = float((x + 1) * S) / float(D)
    i0 = math.floor(lo)
    out = []
    for k in range((S + D - 1) // D + 1):
        w = min(float(i0 + k + 1), hi) - max(float(i0 + k), lo)
        if not w > 0.0:
            w = 0.0
        out.append((min(i0 + k, S - 1), w))
    return out


def rescale(images, size, mode):
    """images uint8 [N, H, W, C], size = (W', H'), mode "average" or "threshold" -> uint8 [N, H', W', C]."""
    N, H, W, C = images.shape
    Wd, Hd = size
    out = np.zeros((N, Hd, Wd, C), np.uint8)
    for y in range(Hd):
        ty = taps(y, H, Hd)
        for x in range(Wd):
            tx = taps(x, W, Wd)
            for n in range(N):
                for c in range(C):
                    acc = A = 0.0
                    for iy, wy in ty:
                        for ix, wx in tx:
                            w = wy * wx
                            acc = acc + w * float(images[n, iy, ix, c])
                            A = A + w
                    v = acc / A
                    out[n, y, x, c] = min(255, math.floor(v + 0.5)) if mode == "average" else (255 if v >= 127.5 else 0)
    return out


def tables():
    """(C, S, HC, HS) as the contract has the host build them: numpy's cos and sin of whole arrays (HC, HS: index j = 1..255)."""
    t = np.arange(256, dtype=np.float64)
    C, S = np.cos(2 * np.pi * t / 255), np.sin(2 * np.pi * t / 255)
    C[255], S[255] = C[0], S[0]
    HC, HS = np.zeros(256), np.zeros(256)
    HC[1:], HS[1:] = np.cos(2 * np.pi * (t[1:] - 0.5) / 255), np.sin(2 * np.pi * (t[1:] - 0.5) / 255)
    return [float(v) for v in C], [float(v) for v in S], [float(v) for v in HC], [float(v) for v in HS]


def upper(x, y):
    return y > 0.0 or (y == 0.0 and x > 0.0)


def pair_bytes(X, Y, Am, tabs):
    """(angle byte, confidence byte) of the sums of one output pixel."""
    _, _, HC, HS = tabs
    conf = 0 if Am == 0.0 else min(255, math.floor(math.sqrt(X * X + Y * Y) / Am + 0.5))
    if X == 0.0 and Y == 0.0:
        return 0, conf
    count = 0
    for j in range(1, 256):
        if upper(X, Y) != upper(HC[j], HS[j]):
            past = upper(HC[j], HS[j])
        else:
            past = HC[j] * Y - HS[j] * X >= 0.0
        count += 1 if past else 0
    return count % 255, conf


def box_sums(t, c, m, w, tabs):
    """(X, Y, Am) of one footprint given as flat lists, in the order the terms are visited (m: None or the mask bytes)."""
    C, S, _, _ = tabs
    X = Y = Am = 0.0
    for i in range(len(t)):
        if m is not None and m[i] == 0:
            continue
        g = w[i] * float(c[i])
        X = X + g * C[t[i]]
        Y = Y + g * S[t[i]]
        Am = Am + w[i]
    return X, Y, Am


def rescale_orientation(angle, conf, mask, size, tabs=None):
    """angle, conf uint8 [N, H, W], mask uint8 [N, H, W] or None, size = (W', H') -> (angle', confidence') uint8 [N, H', W']."""
    tabs = tables() if tabs is None else tabs
    N, H, W = angle.shape
    Wd, Hd = size
    out_t, out_c = np.zeros((N, Hd, Wd), np.uint8), np.zeros((N, Hd, Wd), np.uint8)
    for y in range(Hd):
        ty = taps(y, H, Hd)
        for x in range(Wd):
            tx = taps(x, W, Wd)
            for n in range(N):
                t, c, m, w = [], [], None if mask is None else [], []
                for iy, wy in ty:
                    for ix, wx in tx:
                        t.append(int(angle[n, iy, ix]))
                        c.append(int(conf[n, iy, ix]))
                        w.append(wy * wx)
                        if mask is not None:
                            m.append(int(mask[n, iy, ix]))
                out_t[n, y, x], out_c[n, y, x] = pair_bytes(*box_sums(t, c, m, w, tabs), tabs)
    return out_t, out_c
