"""CPU: PLY IO (c3dgs_amd/ply.py) -- ascii and both binary byte orders, every scalar type, skipped and ignored
elements, each malformed-file error, and the exact header the reference's save_ply writes through plyfile."""
import numpy as np
import pytest

from c3dgs_amd import ply

TYPES = [("char", "i1"), ("uchar", "u1"), ("short", "i2"), ("ushort", "u2"), ("int", "i4"), ("uint", "u4"),
         ("float", "f4"), ("double", "f8"), ("int8", "i1"), ("uint8", "u1"), ("int16", "i2"), ("uint16", "u2"),
         ("int32", "i4"), ("uint32", "u4"), ("float32", "f4"), ("float64", "f8")]


def _columns(n, seed=0):
    g = np.random.default_rng(seed)
    cols = {"x": g.normal(size=n).astype(np.float32), "y": g.normal(size=n).astype(np.float32),
            "z": g.normal(size=n).astype(np.float32)}
    for k, (name, code) in enumerate(TYPES):
        dt = np.dtype(code)
        if dt.kind == "f":
            v = (g.normal(size=n) * 10 ** (k % 5)).astype(dt)
        else:
            info = np.iinfo(dt)
            v = g.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dt)
            v[0], v[-1] = info.min, info.max
        cols[f"p_{name}"] = v
    return cols


def _write(path, fmt, cols, before=None, after=None, crlf=False, comments=True, list_before=False):
    """Assemble a PLY file by hand: optional scalar element before `vertex`, an element after it."""
    n = len(cols["x"])
    types = {"x": "float", "y": "float", "z": "float"}
    types.update({k: k[2:] for k in cols if k.startswith("p_")})
    nl = "\r\n" if crlf else "\n"
    h = ["ply", f"format {fmt} 1.0"]
    if comments:
        h += ["comment written by hand", "obj_info test file"]
    if before is not None:
        h += [f"element camera {len(before)}", "property float fx", "property uchar id"]
        if list_before:
            h += ["property list uchar int idx"]
    h += [f"element vertex {n}"] + [f"property {types[k]} {k}" for k in cols]
    if after is not None:
        h += [f"element face {after}", "property list uchar int vertex_indices"]
    h += ["end_header"]
    head = (nl.join(h) + nl).encode()
    if fmt == "ascii":
        body = []
        if before is not None:
            body += [f"{fx!r} {cid}" + (" 2 7 8" if list_before else "") for fx, cid in before]
        for i in range(n):
            vals = []
            for k in cols:
                v = cols[k][i]
                vals.append(repr(float(v)) if np.dtype(cols[k].dtype).kind == "f" else str(int(v)))
            body.append(" ".join(vals))
        if after is not None:
            body += ["3 0 1 2"] * after
        data = (nl.join(body) + nl).encode()
    else:
        e = "<" if fmt == "binary_little_endian" else ">"
        data = b""
        if before is not None:
            bt = np.dtype([("fx", e + "f4"), ("id", "u1")])
            data += np.array(before, dtype=bt).tobytes()
        dt = np.dtype([(k, e + cols[k].dtype.str[1:]) for k in cols])
        rec = np.empty(n, dtype=dt)
        for k in cols:
            rec[k] = cols[k]
        data += rec.tobytes()
        if after is not None:
            data += (np.array([3], np.uint8).tobytes() + np.array([0, 1, 2], e + "i4").tobytes()) * after
    path.write_bytes(head + data)
    return path


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_round_trip_every_type(tmp_path, fmt):
    cols = _columns(37)
    got = ply.read_ply(_write(tmp_path / "a.ply", fmt, cols))
    assert list(got) == list(cols)
    for k, v in cols.items():
        assert got[k].dtype == v.dtype, k
        np.testing.assert_array_equal(got[k], v, err_msg=k)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_comments_skipped_elements_and_trailing_elements(tmp_path, fmt):
    cols = _columns(9, seed=3)
    before = [(1.5, 3), (-2.25, 200)]
    got = ply.read_ply(_write(tmp_path / "b.ply", fmt, cols, before=before, after=4, crlf=(fmt == "ascii")))
    for k, v in cols.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)


def test_crlf_header_binary(tmp_path):
    cols = _columns(5, seed=4)
    got = ply.read_ply(_write(tmp_path / "c.ply", "binary_little_endian", cols, crlf=True))
    np.testing.assert_array_equal(got["p_double"], cols["p_double"])


def test_ascii_list_element_before_vertex_is_skipped(tmp_path):
    cols = _columns(4, seed=5)
    got = ply.read_ply(_write(tmp_path / "d.ply", "ascii", cols, before=[(1.0, 1)], list_before=True))
    np.testing.assert_array_equal(got["x"], cols["x"])


def test_empty_vertex_element(tmp_path):
    p = tmp_path / "e.ply"
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                  b"property float z\nend_header\n")
    got = ply.read_ply(p)
    assert all(got[k].shape == (0,) for k in "xyz")


def _err(tmp_path, data, match):
    p = tmp_path / "bad.ply"
    p.write_bytes(data)
    with pytest.raises(ValueError, match=match):
        ply.read_ply(p)


def test_errors(tmp_path):
    xyz = b"property float x\nproperty float y\nproperty float z\n"
    _err(tmp_path, b"OFF\n3 1 0\n", "not a PLY")
    _err(tmp_path, b"", "not a PLY")
    _err(tmp_path, b"ply\nformat binary_middle_endian 1.0\nelement vertex 1\n" + xyz + b"end_header\n", "format")
    _err(tmp_path, b"ply\nformat ascii 2.0\nelement vertex 1\n" + xyz + b"end_header\n", "format")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float128 x\nend_header\n", "unknown PLY type")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 1\nproperty list uchar quad x\nend_header\n", "unknown PLY type")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n3 0 1 2\n",
         "no vertex element")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n1 2\n",
         "no 'z' property")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 1\n" + xyz, "end_header")
    _err(tmp_path, b"ply\nelement vertex 1\n" + xyz + b"end_header\n", "no format")
    # truncated bodies
    _err(tmp_path, b"ply\nformat binary_little_endian 1.0\nelement vertex 3\n" + xyz + b"end_header\n" + bytes(30),
         "truncated")
    _err(tmp_path, b"ply\nformat binary_big_endian 1.0\nelement vertex 1\n" + xyz + b"end_header\n", "truncated")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 3\n" + xyz + b"end_header\n1 2 3\n4 5 6\n", "truncated")
    _err(tmp_path, b"ply\nformat ascii 1.0\nelement vertex 2\n" + xyz + b"end_header\n1 2 3\n4 5\n", "expected")
    # a list element before the vertices of a binary file cannot be skipped without parsing it
    _err(tmp_path, b"ply\nformat binary_little_endian 1.0\nelement face 1\nproperty list uchar int vertex_indices\n"
         b"element vertex 1\n" + xyz + b"end_header\n" + bytes(13 + 12), "list property")


def test_write_header_matches_reference_layout(tmp_path):
    # construct_list_of_attributes of a degree-3 model (scene/gaussian_model.py:324-337), as plyfile writes it
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(45)] + \
        ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    n = 11
    g = np.random.default_rng(1)
    cols = {k: g.normal(size=n).astype(np.float32) for k in names}
    p = tmp_path / "w.ply"
    ply.write_ply(p, cols)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 11\n"
    for k in names:
        head += "property float " + k + "\n"
    head += "end_header\n"
    raw = p.read_bytes()
    assert raw[:len(head)] == head.encode("ascii")
    assert len(raw) == len(head) + n * 4 * len(names)
    body = np.frombuffer(raw[len(head):], dtype="<f4").reshape(n, len(names))
    for k, name in enumerate(names):
        np.testing.assert_array_equal(body[:, k], cols[name])
    back = ply.read_ply(p)
    assert list(back) == names
    np.testing.assert_array_equal(back["rot_3"], cols["rot_3"])


def test_write_rejects_ragged_columns(tmp_path):
    with pytest.raises(ValueError, match="shape"):
        ply.write_ply(tmp_path / "r.ply", {"x": np.zeros(3), "y": np.zeros(4), "z": np.zeros(3)})
