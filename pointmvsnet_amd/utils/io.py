"""File formats of the evaluation output: PFM maps and DTU camera text files.

Same function names, signatures and BYTES as reference utils/io.py:15-145 (``load_cam_dtu``, ``write_cam_dtu``,
``load_pfm``, ``write_pfm``, ``mkdir``) -- what ``tools/depthfusion.py`` and fusibile read back.  Written from
the format, not from the reference's code; tests/test_eval_output.py compares against files the reference's own
writers produced (tests/golden/make_eval_golden.py).
"""
import os
import re
import sys

import numpy as np


def mkdir(path):
    os.makedirs(path, exist_ok=True)


def pfm_header(width, height, color=False, scale=1.0, little_endian=True):
    """b'Pf\\n<w> <h>\\n<scale>\\n': a negative scale marks little-endian samples."""
    return b"%s\n%d %d\n%f\n" % (b"PF" if color else b"Pf", width, height, -scale if little_endian else scale)


def write_pfm_body(file, body, width, height, scale=1):
    """Header + ``body`` = the samples already in file order (bottom row first, little-endian float32): what the
    device-side packers of csrc/eval_out.hip produce."""
    with open(file, "wb") as f:
        f.write(pfm_header(width, height, False, float(scale), True))
        f.write(body)


def write_pfm(file, image, scale=1):
    image = np.asarray(image)
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    if image.ndim == 3 and image.shape[2] == 3:
        color = True
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        color = False
    else:
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    little = image.dtype.byteorder == "<" or (image.dtype.byteorder == "=" and sys.byteorder == "little")
    with open(file, "wb") as f:
        f.write(pfm_header(image.shape[1], image.shape[0], color, float(scale), little))
        f.write(np.ascontiguousarray(image[::-1]).tobytes())          # rows bottom-up


def load_pfm(file):
    with open(file, "rb") as f:
        kind = f.readline().rstrip().decode("ascii")
        if kind not in ("PF", "Pf"):
            raise Exception("Not a PFM file.")
        dims = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("ascii"))
        if not dims:
            raise Exception("Malformed PFM header.")
        width, height = int(dims.group(1)), int(dims.group(2))
        scale = float(f.readline().decode("ascii").rstrip())
        endian = "<" if scale < 0 else ">"
        # np.fromfile like the reference (utils/io.py:96): the caller gets a WRITABLE array -- depthfusion.py's
        # probability_filter masks the loaded depth map in place (tools/depthfusion.py:165-168)
        data = np.fromfile(f, dtype=endian + "f4")
    shape = (height, width, 3) if kind == "PF" else (height, width)
    return np.flipud(data.reshape(shape)), abs(scale)


def load_cam_dtu(file, num_depth=0, interval_scale=1.0):
    """(2,4,4): [0] extrinsic, [1][:3,:3] intrinsic, [1][3] = (depth_min, interval, num_depth, depth_max)."""
    words = file.read().split()
    cam = np.zeros((2, 4, 4))
    cam[0] = np.array(words[1:17], dtype=np.float64).reshape(4, 4)
    cam[1, :3, :3] = np.array(words[18:27], dtype=np.float64).reshape(3, 3)
    n = len(words)
    if n in (29, 30, 31):
        cam[1, 3, 0] = float(words[27])
        cam[1, 3, 1] = float(words[28]) * interval_scale
        cam[1, 3, 2] = num_depth if n == 29 else float(words[29])
        cam[1, 3, 3] = float(words[30]) if n == 31 else cam[1, 3, 0] + cam[1, 3, 1] * (num_depth - 1)
    return cam


def cam_dtu_text(cam):
    """The text write_cam_dtu writes: every number through str() (NumPy's shortest round-trip repr)."""
    out = ["extrinsic\n"]
    for i in range(4):
        out.append("".join(str(cam[0][i][j]) + " " for j in range(4)) + "\n")
    out.append("\nintrinsic\n")
    for i in range(3):
        out.append("".join(str(cam[1][i][j]) + " " for j in range(3)) + "\n")
    out.append("\n" + " ".join(str(cam[1][3][j]) for j in range(4)) + "\n")
    return "".join(out)


def write_cam_dtu(file, cam):
    with open(file, "w") as f:
        f.write(cam_dtu_text(cam))


def write_ply(file, points, colors=None, normals=None, faces=None):
    """Binary little-endian PLY of a point cloud: ``x y z`` float32 per vertex, then ``nx ny nz`` float32 when ``normals``
    (N, 3) is given, then ``red green blue`` uchar when ``colors`` (N, 3) is given -- the vertex layout fusibile's
    final3d_model.ply carries; without normals, that layout minus the normals.  With ``faces`` (F, 3), integer rows into
    ``points``, a mesh: ``element face F`` with ``property list uchar int vertex_indices`` follows the vertex element, and
    its records (a count byte 3, three int32) the vertices; without ``faces`` the bytes are those of the cloud."""
    points = np.ascontiguousarray(points, dtype="<f4")
    if points.ndim != 2 or points.shape[1] != 3:
        raise Exception("Points must have N x 3 dimensions.")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype="<f4")
        if normals.shape != points.shape:
            raise Exception("Normals must have the shape of the points.")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != points.shape or colors.dtype != np.uint8:
            raise Exception("Colors must be uint8 with the shape of the points.")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    vertex = np.empty(points.shape[0], dtype=np.dtype(fields))
    for c, n in enumerate("xyz"):
        vertex[n] = points[:, c]
    if normals is not None:
        for c, n in enumerate(("nx", "ny", "nz")):
            vertex[n] = normals[:, c]
    if colors is not None:
        for c, n in enumerate(("red", "green", "blue")):
            vertex[n] = colors[:, c]
    face = None
    if faces is not None:
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
            raise Exception("Faces must be integers with F x 3 dimensions.")
        if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= points.shape[0]):
            raise Exception("Faces must index the points.")
        face = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        face["n"] = 3
        face["v"] = faces
        header += "element face %d\nproperty list uchar int vertex_indices\n"
    with open(file, "wb") as f:
        f.write((header % ((points.shape[0],) + (() if face is None else (face.shape[0],))) + "end_header\n").encode("ascii"))
        f.write(vertex.tobytes())
        if face is not None:
            f.write(face.tobytes())


def load_ply_mesh(file):
    """``(points (N, 3) float32, colours (N, 3) uint8 or None, normals (N, 3) float32 or None, faces (F, 3) int32)`` of a
    PLY file as ``write_ply`` writes it, with or without faces (a cloud gives ``faces`` of shape (0, 3)).  Only triangles
    are read."""
    with open(file, "rb") as f:
        if f.readline().strip() != b"ply":
            raise Exception("Not a PLY file.")
        elements = []                                   # (name, count, [property words])
        while True:
            line = f.readline()
            if not line:
                raise Exception("Malformed PLY header.")
            words = line.decode("ascii").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words == ["end_header"]:
                break
            if words[0] == "format" and words[1:] != ["binary_little_endian", "1.0"]:
                raise Exception("Only binary_little_endian 1.0 PLY files are read.")
            if words[0] == "element":
                elements.append((words[1], int(words[2]), []))
            if words[0] == "property" and elements:
                elements[-1][2].append(tuple(words[1:]))
        xyz = [("float", n) for n in "xyz"]
        nrm = [("float", n) for n in ("nx", "ny", "nz")]
        rgb = [("uchar", n) for n in ("red", "green", "blue")]
        names = [e[0] for e in elements]
        if names not in (["vertex"], ["vertex", "face"]) or elements[0][2] not in (xyz, xyz + rgb, xyz + nrm, xyz + nrm + rgb):
            raise Exception("Only x y z float [nx ny nz float] [red green blue uchar] vertices, then faces, are read.")
        if len(elements) == 2 and elements[1][2] not in ([("list", "uchar", "int", "vertex_indices")],
                                                         [("list", "uchar", "int", "vertex_index")]):
            raise Exception("Only faces of property list uchar int vertex_indices are read.")
        count, props = elements[0][1], elements[0][2]
        dtype = np.dtype([(n, "<f4" if t == "float" else "u1") for t, n in props])
        blob = f.read(count * dtype.itemsize)
        if len(blob) != count * dtype.itemsize:
            raise Exception("Truncated PLY file.")
        vertex = np.frombuffer(blob, dtype=dtype, count=count)
        faces = np.zeros((0, 3), np.int32)
        if len(elements) == 2:
            fdtype = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
            blob = f.read(elements[1][1] * fdtype.itemsize)
            if len(blob) != elements[1][1] * fdtype.itemsize:
                raise Exception("Truncated PLY file.")
            face = np.frombuffer(blob, dtype=fdtype, count=elements[1][1])
            if (face["n"] != 3).any():
                raise Exception("Only triangles are read.")
            faces = np.ascontiguousarray(face["v"], dtype=np.int32).reshape(-1, 3)
            if faces.size and (faces.min() < 0 or faces.max() >= count):
                raise Exception("A face indexes no vertex.")

    def columns(cols, kind):
        return np.stack([vertex[n] for n in cols], axis=1) if count else np.zeros((0, 3), kind)

    have = [n for _, n in props]
    return (columns("xyz", np.float32), columns(("red", "green", "blue"), np.uint8) if "red" in have else None,
            columns(("nx", "ny", "nz"), np.float32) if "nx" in have else None, faces)


def load_ply(file, return_normals=False):
    """(points (N, 3) float32, colors (N, 3) uint8 or None) of a PLY file as ``write_ply`` writes it; with
    ``return_normals`` a third value, the normals (N, 3) float32, or None if the file has none."""
    with open(file, "rb") as f:
        if f.readline().strip() != b"ply":
            raise Exception("Not a PLY file.")
        count, props = None, []
        while True:
            line = f.readline()
            if not line:
                raise Exception("Malformed PLY header.")
            words = line.decode("ascii").split()
            if words == ["end_header"]:
                break
            if words[0] == "format" and words[1:] != ["binary_little_endian", "1.0"]:
                raise Exception("Only binary_little_endian 1.0 PLY files are read.")
            if words[0] == "element":
                if words[1] != "vertex" or count is not None:
                    raise Exception("Only PLY files with one vertex element are read.")
                count = int(words[2])
            if words[0] == "property":
                props.append((words[1], words[2]))
        xyz = [("float", n) for n in "xyz"]
        nrm = [("float", n) for n in ("nx", "ny", "nz")]
        rgb = [("uchar", n) for n in ("red", "green", "blue")]
        if count is None or props not in (xyz, xyz + rgb, xyz + nrm, xyz + nrm + rgb):
            raise Exception("Only x y z float [nx ny nz float] [red green blue uchar] vertices are read.")
        dtype = np.dtype([(n, "<f4" if t == "float" else "u1") for t, n in props])
        vertex = np.frombuffer(f.read(count * dtype.itemsize), dtype=dtype, count=count)
    names = [n for _, n in props]
    points = np.stack([vertex[n] for n in "xyz"], axis=1) if count else np.zeros((0, 3), np.float32)
    colors = normals = None
    if "red" in names:
        colors = np.stack([vertex[n] for n in ("red", "green", "blue")], axis=1) if count else np.zeros((0, 3), np.uint8)
    if "nx" in names:
        normals = np.stack([vertex[n] for n in ("nx", "ny", "nz")], axis=1) if count else np.zeros((0, 3), np.float32)
    return (points, colors, normals) if return_normals else (points, colors)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4",
              "float32": "<f4", "double": "<f8", "float64": "<f8"}


def load_ply_points(file):
    """(N, 3) float32 ``x y z`` of a binary-little-endian PLY whose FIRST element is ``vertex`` with any scalar properties
    (fusibile's clouds and DTU's ``stlNNN_total.ply`` carry normals and colours); later elements such as faces are ignored."""
    with open(file, "rb") as f:
        if f.readline().strip() != b"ply":
            raise Exception("Not a PLY file.")
        elements = []                                   # (name, count, [(type, name)])
        while True:
            line = f.readline()
            if not line:
                raise Exception("Malformed PLY header.")
            words = line.decode("ascii").split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words == ["end_header"]:
                break
            if words[0] == "format" and words[1:] != ["binary_little_endian", "1.0"]:
                raise Exception("Only binary_little_endian 1.0 PLY files are read.")
            if words[0] == "element":
                elements.append((words[1], int(words[2]), []))
            if words[0] == "property" and elements:
                if len(elements) == 1 and (words[1] == "list" or words[1] not in _PLY_TYPES):
                    raise Exception("Only scalar vertex properties are read.")
                elements[-1][2].append((words[1], words[-1]))
        if not elements or elements[0][0] != "vertex":
            raise Exception("The first PLY element must be vertex.")
        _, count, props = elements[0]
        names = [n for _, n in props]
        if any(c not in names for c in "xyz") or len(set(names)) != len(names):
            raise Exception("The PLY vertices need x, y and z.")
        dtype = np.dtype([(n, _PLY_TYPES[t]) for t, n in props])
        blob = f.read(count * dtype.itemsize)
        if len(blob) != count * dtype.itemsize:
            raise Exception("Truncated PLY file.")
        vertex = np.frombuffer(blob, dtype=dtype, count=count)
    if not count:
        return np.zeros((0, 3), np.float32)
    return np.ascontiguousarray(np.stack([vertex[n] for n in "xyz"], axis=1), dtype=np.float32)


def load_dtu_obs_mask(path, mask_name="ObsMask", bb_name="BB", res_name="Res"):
    """``(mask (X, Y, Z) bool, bb_min (3,) float64, res float)`` from DTU's ``ObsMask/ObsMask<scan>_10.mat``: the variables
    ``ObsMask``, ``BB`` (2 x 3, first row the minimum) and ``Res`` as DTU's evaluation program reads them.  Needs SciPy."""
    from scipy.io import loadmat
    mat = loadmat(path)
    for name in (mask_name, bb_name, res_name):
        if name not in mat:
            raise KeyError("%s: no variable %r (has %s)" % (path, name, sorted(k for k in mat if not k.startswith("__"))))
    mask = np.ascontiguousarray(np.asarray(mat[mask_name]) != 0)
    bb = np.asarray(mat[bb_name], dtype=np.float64)
    if mask.ndim != 3 or bb.shape != (2, 3):
        raise ValueError("%s: %s must be a 3-D grid and %s 2 x 3" % (path, mask_name, bb_name))
    return mask, bb[0].copy(), float(np.asarray(mat[res_name], dtype=np.float64).reshape(-1)[0])


def load_dtu_plane(path, plane_name="P"):
    """The four plane floats ``P`` of DTU's ``ObsMask/Plane<scan>.mat`` as a (4,) float64 array.  Needs SciPy."""
    from scipy.io import loadmat
    mat = loadmat(path)
    if plane_name not in mat:
        raise KeyError("%s: no variable %r" % (path, plane_name))
    plane = np.asarray(mat[plane_name], dtype=np.float64).reshape(-1)
    if plane.size != 4:
        raise ValueError("%s: %s must have four values" % (path, plane_name))
    return plane
