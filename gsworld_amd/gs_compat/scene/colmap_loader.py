"""``scene.colmap_loader``: readers of a COLMAP sparse model (``cameras`` / ``images`` / ``points3D``, ``.bin`` or
``.txt``), written from the file layouts COLMAP documents.  Binary files are little-endian throughout.

    cameras.bin   uint64 n; per camera  int32 id, int32 model_id, uint64 width, uint64 height, double params[]
    images.bin    uint64 n; per image   int32 id, double qvec[4] (w,x,y,z), double tvec[3], int32 camera_id,
                                        NUL-terminated name, uint64 m, m x (double x, double y, int64 point3D_id)
    points3D.bin  uint64 n; per point   uint64 id, double xyz[3], uint8 rgb[3], double error, uint64 track_len,
                                        track_len x (int32 image_id, int32 point2D_idx)
"""
import collections
import struct

import numpy as np

CameraModel = collections.namedtuple("CameraModel", ["model_id", "model_name", "num_params"])
Camera = collections.namedtuple("Camera", ["id", "model", "width", "height", "params"])
BaseImage = collections.namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])
Point3D = collections.namedtuple("Point3D", ["id", "xyz", "rgb", "error", "image_ids", "point2D_idxs"])

CAMERA_MODELS = {
    CameraModel(0, "SIMPLE_PINHOLE", 3), CameraModel(1, "PINHOLE", 4), CameraModel(2, "SIMPLE_RADIAL", 4),
    CameraModel(3, "RADIAL", 5), CameraModel(4, "OPENCV", 8), CameraModel(5, "OPENCV_FISHEYE", 8),
    CameraModel(6, "FULL_OPENCV", 12), CameraModel(7, "FOV", 5), CameraModel(8, "SIMPLE_RADIAL_FISHEYE", 4),
    CameraModel(9, "RADIAL_FISHEYE", 5), CameraModel(10, "THIN_PRISM_FISHEYE", 12),
}
CAMERA_MODEL_IDS = {m.model_id: m for m in CAMERA_MODELS}
CAMERA_MODEL_NAMES = {m.model_name: m for m in CAMERA_MODELS}
UNDISTORTED_ONLY = ("Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) "
                    "supported!")


def qvec2rotmat(qvec):
    w, x, y, z = (float(v) for v in qvec)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def rotmat2qvec(R):
    Rxx, Ryx, Rzx, Rxy, Ryy, Rzy, Rxz, Ryz, Rzz = np.asarray(R, dtype=np.float64).flat
    K = np.array([[Rxx - Ryy - Rzz, 0, 0, 0], [Ryx + Rxy, Ryy - Rxx - Rzz, 0, 0], [Rzx + Rxz, Rzy + Ryz, Rzz - Rxx - Ryy, 0],
                  [Ryz - Rzy, Rzx - Rxz, Rxy - Ryx, Rxx + Ryy + Rzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    qvec = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -qvec if qvec[0] < 0 else qvec


class Image(BaseImage):
    def qvec2rotmat(self):
        return qvec2rotmat(self.qvec)


def _unpack(f, fmt):
    fmt = "<" + fmt
    return struct.unpack(fmt, f.read(struct.calcsize(fmt)))


def _check_model(name):
    if name not in ("PINHOLE", "SIMPLE_PINHOLE"):
        raise AssertionError(UNDISTORTED_ONLY)


def read_intrinsics_binary(path):
    cameras = {}
    with open(path, "rb") as f:
        (n,) = _unpack(f, "Q")
        for _ in range(n):
            cam_id, model_id, width, height = _unpack(f, "iiQQ")
            if model_id not in CAMERA_MODEL_IDS:
                raise AssertionError(UNDISTORTED_ONLY)
            model = CAMERA_MODEL_IDS[model_id]
            params = _unpack(f, "d" * model.num_params)
            _check_model(model.model_name)
            cameras[cam_id] = Camera(cam_id, model.model_name, width, height, np.array(params))
    return cameras


def read_intrinsics_text(path):
    cameras = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            e = line.split()
            _check_model(e[1])
            cameras[int(e[0])] = Camera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array([float(v) for v in e[4:]]))
    return cameras


def read_extrinsics_binary(path):
    images = {}
    with open(path, "rb") as f:
        (n,) = _unpack(f, "Q")
        for _ in range(n):
            v = _unpack(f, "idddddddi")
            name = b""
            while True:
                c = f.read(1)
                if c in (b"\x00", b""):
                    break
                name += c
            (m,) = _unpack(f, "Q")
            pts = np.array(_unpack(f, "ddq" * m), dtype=object).reshape(m, 3) if m else np.zeros((0, 3))
            xys = np.array(pts[:, :2], dtype=np.float64).reshape(m, 2)
            ids = np.array(pts[:, 2], dtype=np.int64).reshape(m)
            images[v[0]] = Image(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name.decode("utf-8"), xys, ids)
    return images


def read_extrinsics_text(path):
    images = {}
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f if not ln.lstrip().startswith("#")]
    # two lines per image; the second (the 2D points) may be empty
    while lines and not lines[0].strip():
        lines.pop(0)
    for k in range(0, len(lines) - 1, 2):
        e = lines[k].split()
        if not e:
            break
        p = lines[k + 1].split()
        xys = np.array([[float(p[i]), float(p[i + 1])] for i in range(0, len(p), 3)], dtype=np.float64).reshape(-1, 2)
        ids = np.array([int(p[i + 2]) for i in range(0, len(p), 3)], dtype=np.int64)
        images[int(e[0])] = Image(int(e[0]), np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]),
                                  int(e[8]), " ".join(e[9:]), xys, ids)
    return images


def _points_arrays(points):
    ids = sorted(points)
    if not ids:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 1))
    return (np.array([points[i].xyz for i in ids]), np.array([points[i].rgb for i in ids]),
            np.array([[points[i].error] for i in ids]))


def read_points3D_records_binary(path):
    """-> {id: Point3D} with the tracks (the arrays upstream returns drop them)."""
    points = {}
    with open(path, "rb") as f:
        (n,) = _unpack(f, "Q")
        for _ in range(n):
            v = _unpack(f, "QdddBBBdQ")
            track = _unpack(f, "ii" * v[8])
            points[v[0]] = Point3D(v[0], np.array(v[1:4]), np.array(v[4:7]), v[7], np.array(track[0::2], dtype=np.int64),
                                   np.array(track[1::2], dtype=np.int64))
    return points


def read_points3D_records_text(path):
    points = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            e = line.split()
            track = [int(v) for v in e[8:]]
            points[int(e[0])] = Point3D(int(e[0]), np.array([float(v) for v in e[1:4]]), np.array([int(v) for v in e[4:7]]),
                                        float(e[7]), np.array(track[0::2], dtype=np.int64), np.array(track[1::2], dtype=np.int64))
    return points


def read_points3D_binary(path):
    """-> (xyz (n,3) float64, rgb (n,3), error (n,1)), in the file's order of ids as sorted."""
    return _points_arrays(read_points3D_records_binary(path))


def read_points3D_text(path):
    return _points_arrays(read_points3D_records_text(path))
