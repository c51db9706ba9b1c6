"""Minimal PLY reader / writer (numpy only) for the files the reference exchanges through `plyfile`:
Gaussian clouds (scene/gaussian_model.py:283-412), the five-element strand model (scene/hair_gaussian_model.py:310-466)
and COLMAP point clouds (data/dataset_readers.py:181-213).

Elements are (name, structured array) pairs.  Their properties are scalars, which is all those files contain, or -- for the
face element of the strand export (data/strand_files.py save_ply_faces, the reference's utils/general.py:158-197) -- a sub-array field
such as ("vertex_indices", "<i4", (3,)), written as `property list uchar int vertex_indices` with the count in front of every row, the
way plyfile writes such a field; list properties are read back into such a field when every row has the same count.  Files are
written as `binary_little_endian 1.0` with plyfile's type names (`float`, `int`, `uchar`, ...), i.e. what
`PlyData([...]).write(path)` produces on a little-endian host; binary (either endianness) and ASCII files are read.
SURVEY.md 8f n4: the formats are restated from the cited reference lines; plyfile is not in the image, so no file was
produced by the reference itself ("parity unpinned" for the byte layout; the layout is the public PLY specification)."""
import numpy as np

# PLY scalar type names (both spellings) <-> numpy
_PLY_TO_NP = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_NP_TO_PLY = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float",
              "f8": "double"}


def write_ply(path, elements):
    """elements: iterable of (name, structured ndarray).  One `element` block per pair, in order."""
    header = ["ply", "format binary_little_endian 1.0"]
    blobs = []
    for name, arr in elements:
        arr = np.asarray(arr)
        if arr.dtype.names is None:
            raise TypeError(f"element {name!r}: structured array expected")
        header.append(f"element {name} {arr.shape[0]}")
        fields, counts = [], []
        for f in arr.dtype.names:
            base, shape = arr.dtype[f].base, arr.dtype[f].shape
            code = base.str.lstrip("<>=|")
            if code not in _NP_TO_PLY or len(shape) > 1:
                raise TypeError(f"element {name!r} property {f!r}: unsupported dtype {arr.dtype[f]}")
            if shape:                                             # a fixed-length list: its count in front of every row
                if shape[0] > 255:
                    raise TypeError(f"element {name!r} property {f!r}: {shape[0]} entries do not fit a uchar count")
                header.append(f"property list uchar {_NP_TO_PLY[code]} {f}")
                fields.append((f"{f}\0count", "u1"))
                counts.append((f"{f}\0count", shape[0]))
                fields.append((f, "<" + code, shape))
            else:
                header.append(f"property {_NP_TO_PLY[code]} {f}")
                fields.append((f, "<" + code))
        packed = np.empty(arr.shape[0], dtype=np.dtype(fields))   # packed, little-endian, no padding
        for f in arr.dtype.names:
            packed[f] = arr[f]
        for f, k in counts:
            packed[f] = k
        blobs.append(packed.tobytes())
    header.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        for b in blobs:
            fh.write(b)


def read_ply(path):
    """Returns a list of (name, structured ndarray) in file order."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    lines = data[:end].decode("ascii", "replace").splitlines()
    body = data[nl + 1:]
    fmt, elements = None, []
    for line in lines[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            kinds = tok[2:4] if tok[1] == "list" else tok[1:2]
            for k in kinds:
                if k not in _PLY_TO_NP:
                    raise ValueError(f"{path}: unknown property type {k}")
            # (name, type, count type of a list property or None)
            elements[-1][2].append((tok[4], _PLY_TO_NP[tok[3]], _PLY_TO_NP[tok[2]]) if tok[1] == "list" else (tok[2], _PLY_TO_NP[tok[1]], None))
    if fmt not in ("binary_little_endian", "binary_big_endian", "ascii"):
        raise ValueError(f"{path}: unsupported format {fmt}")

    def ragged(name, p):
        return ValueError(f"{path}: list property {p} of element {name} has rows of different lengths, which are not supported")

    def out_dtype(props, lens):
        return np.dtype([(p, "<" + t) if c is None else (p, "<" + t, (lens[p],)) for p, t, c in props])

    out = []
    if fmt == "ascii":
        tokens = body.split()
        pos = 0
        for name, count, props in elements:
            lens, at = {}, pos                                   # the first row's counts stand for every row's
            for p, t, c in props:
                if c is not None:
                    lens[p] = int(tokens[at]) if count else 0
                    at += 1 + lens[p]
                else:
                    at += 1
            n = at - pos if count else 0
            arr = np.empty(count, dtype=out_dtype(props, lens))
            block = tokens[pos:pos + count * n]
            if len(block) != count * n:
                raise ValueError(f"{path}: truncated element {name}")
            pos += count * n
            conv = lambda col, t: np.array(col, dtype=np.float64).astype(t) if t[0] == "f" else np.array(col, dtype=np.int64).astype(t)
            j = 0
            for p, t, c in props:
                if c is None:
                    try:
                        arr[p] = conv(block[j::n], t)
                    except ValueError:                            # (a float where an integer column was expected, ...)
                        if lens:                                  # the columns of rows of different lengths do not line up
                            raise ragged(name, next(iter(lens))) from None
                        raise
                    j += 1
                    continue
                try:
                    same = not count or bool(np.all(conv(block[j::n], "i8") == lens[p]))
                    for q in range(lens[p] if same else 0):
                        arr[p][:, q] = conv(block[j + 1 + q::n], t)
                except ValueError:
                    same = False
                if not same:
                    raise ragged(name, p)
                j += 1 + lens[p]
            out.append((name, arr))
        if pos != len(tokens) and any(c is not None for _, _, props in elements for _, _, c in props):
            raise ValueError(f"{path}: values left over behind the last element (list rows of different lengths are not supported)")
        return out
    e = "<" if fmt == "binary_little_endian" else ">"
    off = 0
    for name, count, props in elements:
        fields, lens, at = [], {}, off
        for p, t, c in props:
            if c is not None:
                cdt = np.dtype(e + c)
                if count and at + cdt.itemsize > len(body):
                    raise ValueError(f"{path}: truncated element {name}")
                lens[p] = int(np.frombuffer(body, dtype=cdt, count=1, offset=at)[0]) if count else 0
                fields.append((f"{p}\0count", e + c))
                fields.append((p, e + t, (lens[p],)))
                at += cdt.itemsize + lens[p] * np.dtype(t).itemsize
            else:
                fields.append((p, e + t))
                at += np.dtype(t).itemsize
        dt = np.dtype(fields)
        nbytes = dt.itemsize * count
        if off + nbytes > len(body):
            raise (ragged(name, next(iter(lens))) if lens else ValueError(f"{path}: truncated element {name}"))
        arr = np.frombuffer(body, dtype=dt, count=count, offset=off)
        off += nbytes
        if not lens:
            out.append((name, arr.astype(dt.newbyteorder("<")) if e == ">" else arr.copy()))
            continue
        res = np.empty(count, dtype=out_dtype(props, lens))
        for p, t, c in props:
            if c is not None and not np.all(arr[f"{p}\0count"] == lens[p]):
                raise ragged(name, p)
            res[p] = arr[p]
        out.append((name, res))
    if off != len(body) and any(c is not None for _, _, props in elements for _, _, c in props):
        raise ValueError(f"{path}: bytes left over behind the last element (list rows of different lengths are not supported)")
    return out


def element(elements, name):
    for n, a in elements:
        if n == name:
            return a
    raise KeyError(name)


def table(columns, names, dtype="f4"):
    """[N,len(names)] array -> structured array with one scalar property per column."""
    columns = np.asarray(columns)
    arr = np.empty(columns.shape[0], dtype=np.dtype([(n, dtype) for n in names]))
    for j, n in enumerate(names):
        arr[n] = columns[:, j]
    return arr
