"""PLY IO for Gaussian scenes and point clouds, host side, numpy only.

    read_ply(path) -> {property name: np.ndarray[N]}      the `vertex` element of an ascii / binary PLY 1.0 file
    write_ply(path, columns)                               float32 binary little-endian `vertex` element
    write_mesh_ply(path, vertices, colors, faces)          a coloured triangle mesh (c3dgs_amd/mesh.py), binary little-endian
    read_mesh_ply(path) -> (vertices, colors, faces)       what write_mesh_ply wrote

The reference reads and writes these files with `plyfile` (GaussianModel.load_ply / save_ply,
scene/gaussian_model.py:324-503). write_ply produces the same bytes plyfile writes for save_ply: the header
`ply / format binary_little_endian 1.0 / element vertex N / property float <name>... / end_header`, then the packed
records. read_ply reads binary bodies through one structured dtype (no per-vertex Python work: a trained 3M-Gaussian
scene is about 750 MB).
"""
import os

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}
_FORMATS = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}
_MAX_HEADER = 1 << 20


class _Element:
    def __init__(self, name, count):
        self.name, self.count = name, count
        self.props = []                  # (name, numpy type code) of scalar properties
        self.has_list = False


def _header(f, path):
    first = f.readline(16)
    if first.rstrip(b"\r\n") != b"ply":
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic line)")
    fmt, elements, size = None, [], len(first)
    while True:
        raw = f.readline(_MAX_HEADER)
        size += len(raw)
        if not raw or size > _MAX_HEADER:
            raise ValueError(f"{path}: PLY header has no end_header line")
        words = raw.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        key = words[0]
        if key == "end_header":
            break
        if key == "format":
            if len(words) != 3 or words[1] not in _FORMATS or words[2] != "1.0":
                raise ValueError(f"{path}: unsupported PLY format line {raw.strip()!r}")
            fmt = words[1]
        elif key == "element":
            if len(words) != 3 or not words[2].isdigit():
                raise ValueError(f"{path}: bad element line {raw.strip()!r}")
            elements.append(_Element(words[1], int(words[2])))
        elif key == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            el = elements[-1]
            if len(words) == 5 and words[1] == "list":
                if words[2] not in _TYPES or words[3] not in _TYPES:
                    raise ValueError(f"{path}: unknown PLY type in {raw.strip()!r}")
                el.has_list = True
                el.props.append((words[4], None))
            elif len(words) == 3:
                if words[1] not in _TYPES:
                    raise ValueError(f"{path}: unknown PLY type {words[1]!r}")
                el.props.append((words[2], _TYPES[words[1]]))
            else:
                raise ValueError(f"{path}: bad property line {raw.strip()!r}")
        else:
            raise ValueError(f"{path}: unknown PLY header keyword {key!r}")
    if fmt is None:
        raise ValueError(f"{path}: PLY header has no format line")
    return fmt, elements


def read_ply(path):
    """The `vertex` element of a PLY file as {property name: 1-D array} in the file's property order and types
    (native byte order). Elements before `vertex` are skipped (in a binary file they must have scalar properties only);
    elements after it are ignored. Raises ValueError for anything that is not a readable PLY with x, y, z."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        fmt, elements = _header(f, path)
        names = [e.name for e in elements]
        if "vertex" not in names:
            raise ValueError(f"{path}: PLY file has no vertex element")
        vi = names.index("vertex")
        vert = elements[vi]
        if vert.has_list:
            raise ValueError(f"{path}: list properties in the vertex element are not supported")
        pnames = [n for n, _ in vert.props]
        if len(set(pnames)) != len(pnames):
            raise ValueError(f"{path}: duplicate vertex property names")
        for c in "xyz":
            if c not in pnames:
                raise ValueError(f"{path}: vertex element has no '{c}' property")
        if fmt == "ascii":
            return _read_ascii(f, path, elements[:vi], vert)
        order = _FORMATS[fmt]
        for e in elements[:vi]:
            if e.has_list:
                raise ValueError(f"{path}: element {e.name!r} before 'vertex' has a list property; binary files with "
                                 "list elements before the vertices are not supported")
            skip = e.count * np.dtype([(n, order + t) for n, t in e.props]).itemsize if e.props else 0
            f.seek(skip, os.SEEK_CUR)
        dt = np.dtype([(n, order + t) for n, t in vert.props])
        start = f.tell()
        avail = os.fstat(f.fileno()).st_size - start
        if avail < vert.count * dt.itemsize:
            raise ValueError(f"{path}: truncated PLY body: {vert.count} vertices of {dt.itemsize} bytes need "
                             f"{vert.count * dt.itemsize} bytes, {max(avail, 0)} present")
        data = np.fromfile(f, dtype=dt, count=vert.count)
    return {n: np.ascontiguousarray(data[n]).astype(np.dtype(t), copy=False) for n, t in vert.props}


def _read_ascii(f, path, before, vert):
    for e in before:                                        # one line per element instance
        for _ in range(e.count):
            if not f.readline():
                raise ValueError(f"{path}: truncated PLY body in element {e.name!r}")
    lines = []
    for _ in range(vert.count):
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: truncated PLY body: fewer than {vert.count} vertex lines")
        lines.append(line)
    n = len(vert.props)
    tok = b" ".join(lines).split()
    if len(tok) != n * vert.count:
        raise ValueError(f"{path}: vertex lines hold {len(tok)} values, expected {n} x {vert.count}")
    tok = np.array(tok, dtype=object).reshape(vert.count, n) if vert.count else np.empty((0, n), dtype=object)
    out = {}
    for k, (name, t) in enumerate(vert.props):
        col = [s.decode("ascii") for s in tok[:, k]]
        dt = np.dtype(t)
        try:
            out[name] = (np.array(col, dtype=np.int64) if dt.kind in "iu" else np.array(col, dtype=np.float64)).astype(dt)
        except ValueError as e:
            raise ValueError(f"{path}: bad value in vertex property {name!r}: {e}") from None
    return out


_MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_mesh_ply(path, vertices, colors, faces):
    """A triangle mesh as binary little-endian PLY: `element vertex` with float x y z and uchar red green blue (`colors` [V, 3]
    in [0, 1], clamped and rounded to 0..255; None writes 255), `element face` with `property list uchar int vertex_indices`."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"write_mesh_ply: face indices must be in [0, {len(v)})")
    rec = np.empty(len(v), _MESH_VERTEX)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is None:
        rgb = np.full((len(v), 3), 255, np.uint8)
    else:
        c = np.asarray(colors, np.float64).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_mesh_ply: {len(c)} colours for {len(v)} vertices")
        rgb = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    frec = np.empty(len(f), _MESH_FACE)
    frec["n"] = 3
    frec["v"] = f
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(f)}\n"
              "property list uchar int vertex_indices\nend_header\n")
    with open(os.fspath(path), "wb") as fh:
        fh.write(header.encode("ascii"))
        rec.tofile(fh)
        frec.tofile(fh)


def read_mesh_ply(path):
    """-> (vertices [V, 3] float32, colors [V, 3] uint8, faces [F, 3] int32) of a file write_mesh_ply wrote (binary little-endian,
    exactly its two elements and properties, triangles only). Raises ValueError otherwise."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        fmt, elements = _header(f, path)
        ok = (fmt == "binary_little_endian" and [e.name for e in elements] == ["vertex", "face"]
              and elements[0].props == [(n, _MESH_VERTEX[n].str[1:]) for n in _MESH_VERTEX.names]
              and elements[1].props == [("vertex_indices", None)])
        if not ok:
            raise ValueError(f"{path}: not a mesh PLY in write_mesh_ply's layout")
        rec = np.fromfile(f, _MESH_VERTEX, elements[0].count)
        frec = np.fromfile(f, _MESH_FACE, elements[1].count)
    if len(rec) != elements[0].count or len(frec) != elements[1].count:
        raise ValueError(f"{path}: truncated PLY body")
    if frec.size and (frec["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are supported")
    vertices = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
    colors = np.stack([rec["red"], rec["green"], rec["blue"]], 1)
    return vertices, colors, frec["v"].astype(np.int32).reshape(-1, 3)


def ply_header(names, n):
    """The header write_ply (and plyfile, for the reference's save_ply) writes for float32 columns `names`."""
    props = "".join(f"property float {name}\n" for name in names)
    return f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n{props}end_header\n".encode("ascii")


def write_ply(path, columns):
    """Write {name: array[N]} (insertion order = property order) as float32 binary little-endian `vertex` records."""
    path = os.fspath(path)
    names = list(columns)
    if not names:
        raise ValueError("write_ply: no columns")
    n = len(columns[names[0]])
    rec = np.empty(n, dtype=np.dtype([(name, "<f4") for name in names]))
    for name in names:
        col = np.asarray(columns[name])
        if col.shape != (n,):
            raise ValueError(f"write_ply: column {name!r} has shape {col.shape}, expected ({n},)")
        rec[name] = col
    with open(path, "wb") as f:
        f.write(ply_header(names, n))
        rec.tofile(f)
