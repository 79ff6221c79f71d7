"""Readers for COLMAP sparse models (cameras / images / points3D, binary and text), host side, numpy only.

Written from COLMAP's published file formats (https://colmap.github.io/format.html); names and return shapes are the ones
the reference's scene/colmap_loader.py gives its callers:

    read_intrinsics_binary/text(path) -> {camera_id: Camera(id, model, width, height, params float64[n])}
    read_extrinsics_binary/text(path) -> {image_id: Image(id, qvec float64[4], tvec float64[3], camera_id, name,
                                                          xys float64[n,2], point3D_ids int64[n])}   in file order
    read_points3D_binary/text(path)   -> (xyz float64[N,3], rgb float64[N,3], error float64[N,1])
    qvec2rotmat(qvec)                 -> float64[3,3] of the (w, x, y, z) quaternion

All files are little-endian. Binary layouts:
    cameras.bin   u64 count | { i32 id, i32 model_id, u64 width, u64 height, f64 params[model] }
    images.bin    u64 count | { u32 id, f64 q[4], f64 t[3], u32 camera_id, name '\\0', u64 n, { f64 x, f64 y, i64 point3D_id }[n] }
    points3D.bin  u64 count | { u64 id, f64 xyz[3], u8 rgb[3], f64 error, u64 n, { u32 image_id, u32 point2D_idx }[n] }
The records are of variable length, so a cursor walks the record heads; everything of fixed layout (the 2-D observations of an
image, all point records at once) is read through one structured dtype, as ply.py does, without per-value Python work.
A truncated or malformed file raises ValueError naming the path.
"""
import collections
import os
import struct

import numpy as np

Camera = collections.namedtuple("Camera", ["id", "model", "width", "height", "params"])
Image = collections.namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])

# model id -> (name, number of parameters), src/colmap/sensor/models.h
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}

_CAMERA_HEAD = struct.Struct("<iiQQ")
_IMAGE_HEAD = struct.Struct("<I7dI")
_POINT2D = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
_POINT3D = np.dtype([("id", "<u8"), ("xyz", "<f8", (3,)), ("rgb", "u1", (3,)), ("error", "<f8"), ("n", "<u8")])
assert _POINT2D.itemsize == 24 and _POINT3D.itemsize == 51


def qvec2rotmat(qvec):
    """Rotation matrix of the unit quaternion (w, x, y, z), each entry as 1 - 2 a^2 - 2 b^2 or 2 a b -/+ 2 w c, evaluated left to
    right (CameraInfo.extrinsic is compared to the last bit, so the order of the operations is part of the result)."""
    w, x, y, z = qvec[0], qvec[1], qvec[2], qvec[3]
    return np.array([
        [1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
        [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
        [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


class _Cursor:
    """A whole binary file and a position in it; every read checks what is left."""

    def __init__(self, path):
        self.path = os.fspath(path)
        with open(self.path, "rb") as f:
            self.buf = f.read()
        self.pos = 0

    def fail(self, what):
        raise ValueError(f"{self.path}: {what} (at byte {self.pos} of {len(self.buf)})")

    def need(self, n, what):
        if n < 0 or self.pos + n > len(self.buf):
            self.fail(f"truncated or malformed COLMAP file: {what} needs {n} bytes")

    def unpack(self, st, what):
        self.need(st.size, what)
        out = st.unpack_from(self.buf, self.pos)
        self.pos += st.size
        return out

    def count(self, what):
        n = self.unpack(struct.Struct("<Q"), what)[0]
        if n > len(self.buf):                                   # every record is longer than a byte
            self.fail(f"malformed COLMAP file: {what} of {n}")
        return n

    def array(self, dtype, n, what):
        self.need(n * dtype.itemsize if n <= len(self.buf) else -1, what)
        out = np.frombuffer(self.buf, dtype=dtype, count=n, offset=self.pos)
        self.pos += n * dtype.itemsize
        return out

    def cstring(self, what):
        end = self.buf.find(b"\0", self.pos)
        if end < 0:
            self.fail(f"truncated or malformed COLMAP file: unterminated {what}")
        try:
            s = self.buf[self.pos:end].decode("utf-8")
        except UnicodeDecodeError:
            self.fail(f"malformed COLMAP file: {what} is not UTF-8")
        self.pos = end + 1
        return s


def read_intrinsics_binary(path):
    c = _Cursor(path)
    cameras = {}
    for _ in range(c.count("camera count")):
        cid, model_id, width, height = c.unpack(_CAMERA_HEAD, "camera record")
        if model_id not in CAMERA_MODELS:
            c.fail(f"malformed COLMAP file: unknown camera model id {model_id}")
        name, n = CAMERA_MODELS[model_id]
        params = c.array(np.dtype("<f8"), n, "camera parameters").astype(np.float64)
        cameras[cid] = Camera(id=cid, model=name, width=width, height=height, params=params)
    return cameras


def read_extrinsics_binary(path):
    c = _Cursor(path)
    images = {}
    for _ in range(c.count("image count")):
        head = c.unpack(_IMAGE_HEAD, "image record")
        name = c.cstring("image name")
        obs = c.array(_POINT2D, c.count("2-D point count"), "2-D points")
        images[head[0]] = Image(id=head[0], qvec=np.array(head[1:5]), tvec=np.array(head[5:8]), camera_id=head[8], name=name,
                                xys=np.stack((obs["x"], obs["y"]), axis=1).astype(np.float64),
                                point3D_ids=obs["id"].astype(np.int64))
    return images


def read_points3D_binary(path):
    c = _Cursor(path)
    n = c.count("point count")
    starts = np.empty(n, dtype=np.int64)
    track = struct.Struct("<Q")
    for i in range(n):                                          # the cursor only hops from record head to record head
        starts[i] = c.pos
        c.need(_POINT3D.itemsize, "point record")
        length = track.unpack_from(c.buf, c.pos + _POINT3D.itemsize - 8)[0]
        c.pos += _POINT3D.itemsize
        c.need(8 * length if length <= len(c.buf) else -1, "point track")
        c.pos += 8 * length
    raw = np.frombuffer(c.buf, dtype=np.uint8)
    rec = raw[starts[:, None] + np.arange(_POINT3D.itemsize)].view(_POINT3D)[:, 0] if n else np.empty(0, dtype=_POINT3D)
    return rec["xyz"].astype(np.float64), rec["rgb"].astype(np.float64), rec["error"].astype(np.float64)[:, None]


def _text_lines(path):
    path = os.fspath(path)
    try:
        with open(path, "r") as f:
            return path, f.read().split("\n")
    except UnicodeDecodeError as e:
        raise ValueError(f"{path}: not a COLMAP text file: {e}") from None


def _is_record(line):
    line = line.strip()
    return len(line) > 0 and line[0] != "#"


def read_intrinsics_text(path):
    """cameras.txt: `CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]` per line, `#` comments."""
    path, lines = _text_lines(path)
    cameras = {}
    for no, line in enumerate(lines, 1):
        if not _is_record(line):
            continue
        e = line.split()
        try:
            cid, model, width, height = int(e[0]), e[1], int(e[2]), int(e[3])
            params = np.array([float(v) for v in e[4:]], dtype=np.float64)
        except (IndexError, ValueError):
            raise ValueError(f"{path}: malformed camera on line {no}") from None
        known = {name: n for name, n in CAMERA_MODELS.values()}
        if model not in known or len(params) != known[model]:
            raise ValueError(f"{path}: line {no}: camera model {model!r} with {len(params)} parameters")
        cameras[cid] = Camera(id=cid, model=model, width=width, height=height, params=params)
    return cameras


def read_extrinsics_text(path):
    """images.txt: two lines per image, `IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME`, then `X Y POINT3D_ID` triples (the
    second line may be empty)."""
    path, lines = _text_lines(path)
    images = {}
    no = 0
    while no < len(lines):
        line = lines[no]
        no += 1
        if not _is_record(line):
            continue
        e = line.split()
        obs = lines[no].split() if no < len(lines) else []
        no += 1
        try:
            iid, camera_id, name = int(e[0]), int(e[8]), e[9]
            qvec = np.array([float(v) for v in e[1:5]], dtype=np.float64)
            tvec = np.array([float(v) for v in e[5:8]], dtype=np.float64)
            if len(obs) % 3:
                raise ValueError
            xys = np.array([float(v) for v in obs], dtype=np.float64).reshape(-1, 3)[:, :2].copy()
            ids = np.array([int(v) for v in obs[2::3]], dtype=np.int64)
        except (IndexError, ValueError):
            raise ValueError(f"{path}: malformed image record ending on line {no}") from None
        images[iid] = Image(id=iid, qvec=qvec, tvec=tvec, camera_id=camera_id, name=name, xys=xys, point3D_ids=ids)
    return images


def read_points3D_text(path):
    """points3D.txt: `POINT3D_ID X Y Z R G B ERROR TRACK[]` per line."""
    path, lines = _text_lines(path)
    rows = []
    for no, line in enumerate(lines, 1):
        if not _is_record(line):
            continue
        e = line.split()
        try:
            rows.append([float(v) for v in e[1:4]] + [float(int(v)) for v in e[4:7]] + [float(e[7])])
        except (IndexError, ValueError):
            raise ValueError(f"{path}: malformed point on line {no}") from None
    a = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return a[:, 0:3].copy(), a[:, 3:6].copy(), a[:, 6:7].copy()
