"""Strand files other tools read, written from a StrandExport (scene/strand_export.py: points [N,3], attrs [N,5] = RGB, opacity,
width per point, offsets [K+1], strand_ids [K]):

* Cem Yuksel's .hair (data/cy_hair.py: the layout; www.cemyuksel.com/research/hairmodels): segment counts, points, thickness = the
  width, transparency = 1 - opacity, colours;
* USC-HairSalon's .data: int32 strand count, then per strand an int32 point count and that many float32 xyz -- `read_usc_hair` is
  the plain reader of that layout (data/hair_data.py's dataset loader insists on 10000 strands of 1 or 100 vertices);
* the reference's two MeshLab layouts (utils/general.py:127-197, which scripts/convert_output.py writes): a vertex element `x y z`
  (float) `red green blue` (uchar) with either an `edge` element `vertex1 vertex2` (int) or one triangle (A, midpoint, B) per segment,
  the midpoints appended behind the vertices, as `property list uchar int vertex_indices`;
* an .npz with the keys of hair_eval_data.npz (data/hair_data.py save_hair_eval_data_npz; data/eval_data.py reads it).
None of them is produced by the reference from a model's own strands, nor are .hair / .data written by it at all."""
import struct

import numpy as np

from data.cy_hair import write_cy_hair
from utils.ply import write_ply


def _counts(result):
    off = np.asarray(result.offsets, np.int64)
    return off[1:] - off[:-1]


# ---- .hair / .data ---------------------------------------------------------------------------------------------------------------
def write_strands_cy(path, result, info="hair-gs_amd export"):
    """Every strand with its own segment count (points = segments + 1), thickness, transparency and colours per point."""
    cnt = _counts(result)
    if cnt.size and cnt.min() < 1:
        raise ValueError("write_strands_cy: a strand without points")
    if cnt.size and cnt.max() - 1 > 65535:
        raise ValueError(f"write_strands_cy: a strand of {int(cnt.max()) - 1} segments; the .hair segment count is 16 bits (65535)")
    attrs = np.asarray(result.attrs, np.float32)
    if attrs.shape[1] < 5:
        raise ValueError("write_strands_cy: attributes (red, green, blue, opacity, width) expected")
    write_cy_hair(path, result.points, segments=(cnt - 1).astype(np.uint16), colors=attrs[:, 0:3], info=info[:87],
                  thickness=attrs[:, 4], transparency=np.float32(1.0) - attrs[:, 3])


def write_strands_usc(path, result):
    cnt = _counts(result)
    if cnt.size and cnt.max() > np.iinfo(np.int32).max:
        raise ValueError("write_strands_usc: a strand with more than 2^31 - 1 points")
    pts = np.ascontiguousarray(result.points, "<f4").reshape(-1, 3)
    off = np.asarray(result.offsets, np.int64)
    # one record array per distinct point count would be the fast path; the count words are interleaved by a byte view instead
    words = np.empty(cnt.size + 3 * pts.shape[0], "<u4")
    at = np.arange(cnt.size, dtype=np.int64) + 3 * off[:-1]                  # word position of every strand's count
    mask = np.ones(words.shape[0], bool)
    mask[at] = False
    words[at] = cnt.astype("<i4").view("<u4")
    words[mask] = pts.reshape(-1).view("<u4")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", cnt.size))
        fh.write(words.tobytes())


def read_usc_hair(path):
    """(points float32 [N,3], offsets int64 [K+1]) of a .data file, whatever its strand and vertex counts."""
    with open(path, "rb") as fh:
        buf = fh.read()
    if len(buf) < 4:
        raise ValueError(f"{path}: shorter than the strand count")
    (ns,) = struct.unpack_from("<i", buf, 0)
    if ns < 0:
        raise ValueError(f"{path}: {ns} strands")
    cnt = np.empty(ns, np.int64)
    pos = 4
    chunks = []
    for s in range(ns):
        if pos + 4 > len(buf):
            raise ValueError(f"{path}: truncated at strand {s}")
        (nv,) = struct.unpack_from("<i", buf, pos)
        pos += 4
        if nv < 0 or pos + 12 * nv > len(buf):
            raise ValueError(f"{path}: strand {s} with {nv} vertices does not fit the file")
        chunks.append(np.frombuffer(buf, dtype="<f4", count=3 * nv, offset=pos))
        cnt[s] = nv
        pos += 12 * nv
    pts = np.concatenate(chunks).reshape(-1, 3).astype(np.float32) if chunks else np.zeros((0, 3), np.float32)
    return pts, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


# ---- polylines / triangles for a mesh viewer -------------------------------------------------------------------------------------
def strand_edges(result):
    """[E,2] int32: consecutive points of every strand."""
    off = np.asarray(result.offsets, np.int64)
    n = int(off[-1])
    keep = np.ones(n, bool)
    keep[off[1:][off[1:] > off[:-1]] - 1] = False                           # every strand's last point starts no edge
    a = np.nonzero(keep)[0]
    return np.stack([a, a + 1], axis=1).astype(np.int32)


def strand_colours(result, colour="model"):
    """uint8 [N,3] per point: "model" = the exported RGB (round half to even of 255 x), "strand" = one hue per strand,
    hue = uint8(linspace(0, 180, K)[k]) at full saturation and value through OpenCV's 8-bit HSV -> RGB (data/hair_data.py
    hsv2rgb_u8), the colouring of scripts/convert_output.py."""
    cnt = _counts(result)
    if colour == "model":
        rgb = np.asarray(result.attrs, np.float32)[:, 0:3]
        return np.clip(np.rint(rgb * np.float32(255.0)), 0, 255).astype(np.uint8)
    if colour != "strand":
        raise ValueError(f"colour = {colour!r}: 'model' or 'strand'")
    from data.hair_data import hsv2rgb_u8
    hues = np.linspace(start=0, stop=180, num=cnt.size).astype(np.uint8)
    table = np.stack([hsv2rgb_u8(h) for h in range(181)])                   # (one conversion per possible hue, not per strand)
    return np.repeat(table[hues], cnt, axis=0)


def _vertex_element(xyz, rgb):
    v = np.empty(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for j, name in enumerate(("x", "y", "z")):
        v[name] = xyz[:, j]
    for j, name in enumerate(("red", "green", "blue")):
        v[name] = rgb[:, j]
    return v


def save_ply_edges(vertex_xyz, vertex_color, edges, file_path):
    """Polylines: vertices with colours and an `edge` element (reference utils/general.py:127-155)."""
    els = [("vertex", _vertex_element(np.asarray(vertex_xyz, np.float32), np.asarray(vertex_color)))]
    if edges is not None:
        e = np.empty(len(edges), dtype=[("vertex1", "<i4"), ("vertex2", "<i4")])
        e["vertex1"], e["vertex2"] = np.asarray(edges)[:, 0], np.asarray(edges)[:, 1]
        els.append(("edge", e))
    write_ply(file_path, els)


def save_ply_faces(vertex_xyz, vertex_color, edges, file_path):
    """Every segment (A, B) as the triangle (A, (A + B) / 2, B), for viewers that draw no polylines; the midpoints and their colours
    (the mean of the two ends', cast to uchar) follow the vertices (reference utils/general.py:158-197)."""
    xyz, col, edges = np.asarray(vertex_xyz), np.asarray(vertex_color), np.asarray(edges, np.int64).reshape(-1, 2)
    n = xyz.shape[0]
    seg = xyz[edges]
    mid = (seg[:, 0] + seg[:, 1]) / 2
    mid_col = (col[edges[:, 0]].astype(np.float64) + col[edges[:, 1]].astype(np.float64)) / 2
    xyz = np.concatenate((xyz, mid), axis=0).astype(np.float32)
    col = np.concatenate((col.astype(np.float64), mid_col), axis=0).astype(np.uint8)
    f = np.empty(edges.shape[0], dtype=[("vertex_indices", "<i4", (3,))])
    f["vertex_indices"] = np.column_stack((edges[:, 0], np.arange(edges.shape[0]) + n, edges[:, 1]))
    write_ply(file_path, [("vertex", _vertex_element(xyz, col)), ("face", f)])


def write_strands_ply(path, result, faces=False, colour="model"):
    (save_ply_faces if faces else save_ply_edges)(np.asarray(result.points, np.float32), strand_colours(result, colour),
                                                  strand_edges(result), path)


# ---- hair_eval_data.npz ----------------------------------------------------------------------------------------------------------
def strand_eval_data(result):
    """The export as oriented points (loss/metrics.py HairEvalData): the first point of every segment of the exported polylines, the
    unit direction to the next (float32, as compute_eval_data_from_hair_gs computes it), the strand's number, and the edges between
    consecutive points of a strand.  A segment of length zero has no direction: it is left out (compute_eval_data_from_hair_gs
    keeps it with a NaN direction), and the edge then joins its two neighbours, which meet at the same place.  Without such
    segments the points, directions and strand numbers of a native-mode export are that function's, bit for bit."""
    from loss.metrics import HairEvalData
    pts = np.asarray(result.points, np.float32)
    e = strand_edges(result).astype(np.int64)
    cnt = _counts(result)
    seg = pts[e]
    directions = seg[:, 1] - seg[:, 0]
    norm = np.linalg.norm(directions, axis=1, keepdims=True)
    sid = np.repeat(np.asarray(result.strand_ids).astype(np.int32), np.maximum(cnt - 1, 0))   # (int32, like strands_info.id_to_strand_id)
    keep = norm[:, 0] > 0
    directions, norm, sid, first = directions[keep], norm[keep], sid[keep], e[keep, 0]
    directions /= norm
    a = np.nonzero(sid[:-1] == sid[1:])[0]                  # point q is joined to point q + 1 where both lie on one strand
    return HairEvalData(points=pts[first], directions=directions, points_id_to_strand_id=sid,
                        edges=np.stack([a, a + 1], axis=1).astype(np.int32))


def write_strands_npz(path, result):
    d = strand_eval_data(result)
    with open(path, "wb") as fh:        # (a file object: np.savez appends no ".npz" to the name the caller chose)
        np.savez(fh, points=d.points, directions=d.directions, points_id_to_strand_id=d.points_id_to_strand_id, edges=d.edges)
