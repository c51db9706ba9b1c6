"""Reader of Cem Yuksel's .hair format (www.cemyuksel.com/research/hairmodels; the reference's data/cy_hair.py).

Layout, little-endian: a 128-byte header "<4sIIIIff3f88s" = signature "HAIR", hair count, point count, array bits, default
segment count, default thickness, default transparency, default colour (3 floats), 88 bytes of information text; then, in this
order and only where its bit is set: segments (uint16 per hair, bit 1), points (3 float32 per point, bit 2), thickness (float32
per point, bit 4), transparency (float32 per point, bit 8), colours (3 float32 per point, bit 16)."""
import struct
from typing import NamedTuple, Optional

import numpy as np

SEGMENTS_BIT, POINTS_BIT, THICKNESS_BIT, TRANSPARENCY_BIT, COLORS_BIT = 1, 2, 4, 8, 16
HEADER = struct.Struct("<4sIIIIff3f88s")


class CYHairHeader(NamedTuple):
    hair_count: int
    point_count: int
    arrays: int
    d_segments: int
    d_thickness: float
    d_transparency: float
    d_color: tuple
    info: str


class CYHair(NamedTuple):
    header: CYHairHeader
    segments: Optional[np.ndarray]       # uint16 [hair_count]
    points: Optional[np.ndarray]         # float32 [point_count, 3]
    thickness: Optional[np.ndarray]      # float32 [point_count]
    transparency: Optional[np.ndarray]   # float32 [point_count]
    colors: Optional[np.ndarray]         # float32 [point_count, 3]


def read_cy_hair(path):
    with open(path, "rb") as fh:
        buf = fh.read()
    if len(buf) < HEADER.size:
        raise ValueError(f"{path}: shorter than the 128-byte .hair header")
    sig, nh, npt, arrays, dseg, dth, dtr, r, g, b, info = HEADER.unpack_from(buf, 0)
    if sig != b"HAIR":
        raise ValueError(f"{path}: not a .hair file (signature {sig!r})")
    header = CYHairHeader(nh, npt, arrays, dseg, dth, dtr, (r, g, b), info.split(b"\0", 1)[0].decode("ascii", "replace"))
    pos = HEADER.size

    def take(bit, dtype, count, shape, what):
        nonlocal pos
        if not arrays & bit:
            return None
        n = np.dtype(dtype).itemsize * count
        if pos + n > len(buf):
            raise ValueError(f"{path}: the {what} array is truncated")
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=pos).reshape(shape)
        pos += n
        return a.copy()

    seg = take(SEGMENTS_BIT, "<u2", nh, (nh,), "segments")
    pts = take(POINTS_BIT, "<f4", 3 * npt, (npt, 3), "points")
    th = take(THICKNESS_BIT, "<f4", npt, (npt,), "thickness")
    tr = take(TRANSPARENCY_BIT, "<f4", npt, (npt,), "transparency")
    col = take(COLORS_BIT, "<f4", 3 * npt, (npt, 3), "colors")
    return CYHair(header, seg, pts, th, tr, col)


def write_cy_hair(path, points, segments=None, colors=None, d_segments=0, info="", thickness=None, transparency=None):
    """Writes a .hair file: segments, points and the optional per-point thickness, transparency and colours, in the format's order
    (the fixture helper of the tests and tools, and what data/strand_files.py exports through)."""
    points = np.asarray(points, "<f4").reshape(-1, 3)
    nh = len(segments) if segments is not None else (points.shape[0] // (d_segments + 1) if d_segments else 0)
    arrays = POINTS_BIT | (SEGMENTS_BIT if segments is not None else 0) | (COLORS_BIT if colors is not None else 0) \
        | (THICKNESS_BIT if thickness is not None else 0) | (TRANSPARENCY_BIT if transparency is not None else 0)
    with open(path, "wb") as fh:
        fh.write(HEADER.pack(b"HAIR", nh, points.shape[0], arrays, d_segments, 1.0, 0.0, 1.0, 1.0, 1.0, info.encode("ascii")))
        if segments is not None:
            fh.write(np.asarray(segments, "<u2").tobytes())
        fh.write(points.tobytes())
        for per_point in (thickness, transparency):
            if per_point is not None:
                fh.write(np.asarray(per_point, "<f4").reshape(points.shape[0]).tobytes())
        if colors is not None:
            fh.write(np.asarray(colors, "<f4").reshape(-1, 3).tobytes())
