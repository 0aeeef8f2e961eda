"""Binary little-endian PLY files of the meshes of cmdiad_amd.mesh (docs/mesh.md): the header, an atomic writer, a validating
reader and a small fixed pool of writer threads.  Host only; numpy and the standard library.

A file is the header below, then n_vert vertex records of 35 bytes (VERTEX), then n_face face records of 13 bytes (FACE: the list
length, always 3, and three vertex indices) -- the bytes cmdiad_mesh_write leaves on the device, unchanged.

`read_points` is the way in for anybody's files (docs/organize.md): the vertex element of an ascii or binary little-endian PLY as
a dict of arrays, whatever scalar properties it has.
"""
import os

import numpy as np

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("score", "<f4"), ("region", "<i4")])
FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
VERTEX_BYTES, FACE_BYTES = VERTEX.itemsize, FACE.itemsize          # 35, 13
MARK = "cmdiad_amd mesh 1"
MAX_HEADER = 1 << 16
_PLY_TYPES = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<i4": "int"}


class PlyError(ValueError):
    pass


def _properties():
    return [f"property {_PLY_TYPES[VERTEX[name].str]} {name}" for name in VERTEX.names]


def header(n_vert, n_face, comments=()):
    """The ASCII header ('\\n' line ends) of a file with n_vert vertices and n_face faces.  comments: printable ASCII lines, put
    behind the package's own mark; a newline (or anything else outside 0x20..0x7e) is refused."""
    n_vert, n_face = int(n_vert), int(n_face)
    if n_vert < 0 or n_face < 0:
        raise PlyError(f"ply.header: n_vert = {n_vert}, n_face = {n_face} must not be negative")
    lines = ["ply", "format binary_little_endian 1.0", f"comment {MARK}"]
    for c in comments:
        c = str(c)
        if not all(0x20 <= ord(ch) <= 0x7e for ch in c):
            raise PlyError(f"ply.header: a comment is one line of printable ASCII, got {c!r}")
        lines.append(f"comment {c}")
    lines += [f"element vertex {n_vert}"] + _properties() + [f"element face {n_face}", "property list uchar int vertex_indices",
                                                              "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _payload(data, count, size, what):
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    view = memoryview(data).cast("B")
    if view.nbytes != count * size:
        raise PlyError(f"ply.write: {view.nbytes} bytes of {what} records, {count} records of {size} bytes are {count * size}")
    return view


def write(path, n_vert, vertex_bytes, n_face, face_bytes, comments=()):
    """One file: the header and the two record runs as they are (bytes, a memoryview, or a numpy array of VERTEX / FACE records or
    of bytes).  Atomic: written under a temporary name in the same directory, flushed, then os.replace()d.  Returns the file's size."""
    head = header(n_vert, n_face, comments)
    verts, faces = _payload(vertex_bytes, int(n_vert), VERTEX_BYTES, "vertex"), _payload(face_bytes, int(n_face), FACE_BYTES, "face")
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(head)
            f.write(verts)
            f.write(faces)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return len(head) + verts.nbytes + faces.nbytes


def _parse_header(blob, path):
    """(n_vert, n_face, comments, header length) of a file written by `write`; anything else is refused"""
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise PlyError(f"{path}: not a PLY file with a header of at most {MAX_HEADER} bytes")
    try:
        lines = blob[:end].decode("ascii").split("\n")[:-1]
    except UnicodeDecodeError:
        raise PlyError(f"{path}: the header is not ASCII") from None
    if len(lines) < 3 or lines[1] != "format binary_little_endian 1.0" or lines[2] != f"comment {MARK}":
        raise PlyError(f"{path}: the header does not start with 'format binary_little_endian 1.0' and 'comment {MARK}'")
    at, comments = 3, []
    while at < len(lines) and lines[at].startswith("comment "):
        comments.append(lines[at][len("comment "):])
        at += 1
    want = ["element vertex "] + _properties() + ["element face ", "property list uchar int vertex_indices"]
    rest = lines[at:]
    if len(rest) != len(want):
        raise PlyError(f"{path}: {len(rest)} element and property lines, this package writes {len(want)}")
    counts = []
    for got, exp in zip(rest, want):
        if exp.endswith(" ") and exp.startswith("element"):
            tail = got[len(exp):]
            if not got.startswith(exp) or not tail.isdigit() or len(tail) > 10:
                raise PlyError(f"{path}: bad header line {got!r} (expected '{exp}<count>')")
            counts.append(int(tail))
        elif got != exp:
            raise PlyError(f"{path}: bad header line {got!r} (expected {exp!r})")
    return counts[0], counts[1], comments, end + len(b"end_header\n")


def read(path):
    """(vertices, faces, comments): two numpy structured arrays (VERTEX, FACE) and the caller's comment lines.  The header, the
    counts and the sizes are checked against the file's length BEFORE the payload is touched; then every face must be a triangle
    whose indices lie below n_vert.  Every refusal is a PlyError."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        n_vert, n_face, comments, at = _parse_header(f.read(min(size, MAX_HEADER)), path)
        need = at + n_vert * VERTEX_BYTES + n_face * FACE_BYTES
        if need != size:
            raise PlyError(f"{path}: {n_vert} vertices and {n_face} faces behind a header of {at} bytes are {need} bytes, the file has "
                           f"{size}")
        f.seek(at)
        verts = np.frombuffer(f.read(n_vert * VERTEX_BYTES), dtype=VERTEX)
        faces = np.frombuffer(f.read(n_face * FACE_BYTES), dtype=FACE)
    if len(verts) != n_vert or len(faces) != n_face:
        raise PlyError(f"{path}: the file ended inside the payload")
    if n_face and (np.any(faces["n"] != 3) or faces["vertex_indices"].min() < 0 or faces["vertex_indices"].max() >= n_vert):
        raise PlyError(f"{path}: a face is not a triangle over the file's {n_vert} vertices")
    return verts, faces, comments


# ------------------------------------------------------------------------------------------------ any file's points (docs/organize.md)
_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
            "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
MAX_PROPERTIES = 256


def _points_header(blob, path):
    """(format, n_vert, [(name, numpy type code)], header length) of the vertex element of any PLY header"""
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") and not blob.startswith(b"ply\r\n") or end < 0:
        raise PlyError(f"{path}: not a PLY file with a header of at most {MAX_HEADER} bytes")
    try:
        lines = [ln.strip() for ln in blob[:end].decode("ascii").split("\n")]
    except UnicodeDecodeError:
        raise PlyError(f"{path}: the header is not ASCII") from None
    fmt, element, n_vert, props = None, None, None, []
    for ln in lines[1:]:
        tok = ln.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian") or tok[2] != "1.0":
                raise PlyError(f"{path}: format {' '.join(tok[1:])!r}: ascii 1.0 and binary_little_endian 1.0 are read (not big-endian)")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit() or len(tok[2]) > 12:
                raise PlyError(f"{path}: bad header line {ln!r}")
            if n_vert is not None:
                break                                   # whatever follows the vertex element is not read
            element = tok[1]
            if element == "vertex":
                n_vert = int(tok[2])
        elif tok[0] == "property":
            if len(tok) >= 2 and tok[1] == "list":
                where = "inside the vertex element" if element == "vertex" else f"in element {element!r} in front of the vertices"
                raise PlyError(f"{path}: a list property {where}: the vertices cannot be located without reading the payload")
            if len(tok) != 3 or tok[1] not in _SCALARS:
                raise PlyError(f"{path}: bad header line {ln!r}")
            if element != "vertex":
                raise PlyError(f"{path}: element {element!r} stands in front of the vertices: only files that start with them are read")
            if tok[2] in [p[0] for p in props] or len(props) >= MAX_PROPERTIES:
                raise PlyError(f"{path}: property {tok[2]!r} twice, or more than {MAX_PROPERTIES} properties")
            props.append((tok[2], _SCALARS[tok[1]]))
        else:
            raise PlyError(f"{path}: bad header line {ln!r}")
    if fmt is None or n_vert is None:
        raise PlyError(f"{path}: the header has no format line or no vertex element")
    return fmt, n_vert, props, end + len(b"end_header\n")


def read_points(path):
    """The `vertex` element of an ascii or binary_little_endian PLY file -> {property name: array [N]} in the file's types, except that
    x, y and z (required, float or double) come back as float32: float64 coordinates are rounded.  red / green / blue and an integer
    label are what dataset.PointCloudClass looks for; any further scalar property is returned as well.  Elements behind the vertices
    (faces) are not read.  A list property in or in front of the vertices, any property in front of them, a big-endian file, a count
    the file's size cannot hold and a file that ends early are PlyErrors, raised before the payload is interpreted."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        fmt, n, props, at = _points_header(f.read(min(size, MAX_HEADER)), path)
        names = [p[0] for p in props]
        for c in "xyz":
            if c not in names or dict(props)[c] not in ("f4", "f8"):
                raise PlyError(f"{path}: the vertex element needs float or double x, y and z, it has {names}")
        if "label" in names and dict(props)["label"][0] not in "iu":
            raise PlyError(f"{path}: label must be an integer property")
        f.seek(at)
        if fmt == "binary_little_endian":
            rec = np.dtype([(nm, "<" + t) for nm, t in props])
            if at + n * rec.itemsize > size:
                raise PlyError(f"{path}: {n} vertices of {rec.itemsize} bytes behind a header of {at} bytes are more than the file's "
                               f"{size} bytes")
            data = np.frombuffer(f.read(n * rec.itemsize), dtype=rec)
            if len(data) != n:
                raise PlyError(f"{path}: the file ended inside the vertices")
            cols = {nm: data[nm] for nm in names}
        else:
            if n * 2 * len(props) - 1 > size - at:      # a value and a separator each, at the least
                raise PlyError(f"{path}: {n} vertices of {len(props)} values do not fit the file's {size - at} bytes behind the header")
            rows = []
            for _ in range(n):
                tok = f.readline().split()
                if len(tok) != len(props):
                    raise PlyError(f"{path}: the file ended inside the vertices, or a vertex line has {len(tok)} values for "
                                   f"{len(props)} properties")
                rows.append(tok)
            try:
                cols = {nm: np.array([float(r[k]) if t[0] == "f" else int(r[k]) for r in rows]).astype(t) if n else np.zeros(0, t)
                        for k, (nm, t) in enumerate(props)}
            except (ValueError, OverflowError):
                raise PlyError(f"{path}: a vertex line holds something that is not a number") from None
    out = {nm: np.ascontiguousarray(cols[nm]) for nm in names}
    for c in "xyz":
        out[c] = out[c].astype(np.float32)
    return out


def write_many(paths, n_verts, vertex_rows, n_faces, face_rows, comments=None, writers=4):
    """One file per mesh i at paths[i] (the directories exist): the first n_verts[i] records of vertex_rows[i] and the first
    n_faces[i] of face_rows[i] (rows of bytes on the host: numpy uint8).  comments: None, or one list of lines per file.  `writers`
    threads, a pool of fixed size.  Returns the files' sizes in bytes."""
    import concurrent.futures as cf
    paths = list(paths)
    if not (len(paths) == len(n_verts) == len(vertex_rows) == len(n_faces) == len(face_rows)) or \
            (comments is not None and len(comments) != len(paths)):
        raise PlyError(f"ply.write_many: {len(paths)} paths need as many counts, rows and comment lists")

    def one(i):
        nv, nf = int(n_verts[i]), int(n_faces[i])
        return write(paths[i], nv, np.asarray(vertex_rows[i]).reshape(-1)[:nv * VERTEX_BYTES], nf,
                     np.asarray(face_rows[i]).reshape(-1)[:nf * FACE_BYTES], comments[i] if comments is not None else ())
    if len(paths) <= 1 or writers <= 1:
        return [one(i) for i in range(len(paths))]
    with cf.ThreadPoolExecutor(writers) as pool:
        return list(pool.map(one, range(len(paths))))
