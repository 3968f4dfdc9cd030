"""Binary PLY files of indexed triangle meshes with the standard library and numpy only: the bytes gsdf_hip_indexed_ply packs on
the device (include/gsdf_hip.h), and a reader for them."""
import numpy as np


def header(n_verts, n_faces, normals=False, quality=False):
    """The header as the library writes it: its `comment gsdf` line is padded with spaces so that the length is a multiple of 4.
    quality: one more float per vertex, `property float quality`, behind the normals when there are any (this module's own
    addition; the library's files have none)."""
    a = "ply\nformat binary_little_endian 1.0\ncomment gsdf"
    b = f"\nelement vertex {int(n_verts)}\nproperty float x\nproperty float y\nproperty float z\n"
    if normals:
        b += "property float nx\nproperty float ny\nproperty float nz\n"
    if quality:
        b += "property float quality\n"
    b += f"element face {int(n_faces)}\nproperty list uchar int vertex_indices\nend_header\n"
    return (a + " " * ((4 - (len(a) + len(b)) % 4) % 4) + b).encode("ascii")


def ply_bytes(verts, idx, normals=None, quality=None):
    """The file for verts (V, 3) float32, idx (F, 3) vertex numbers and, optionally, normals (V, 3) float32 and a quality (V,)
    float32 per vertex (a wall thickness, say), carried bit for bit. Without quality: the bytes the library packs."""
    verts = np.ascontiguousarray(verts, "<f4").reshape(-1, 3)
    idx = np.ascontiguousarray(idx).reshape(-1, 3)
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= max(len(verts), 1) or int(idx.max()) >= 2 ** 31):
        raise ValueError("vertex index out of range")
    if normals is not None:
        normals = np.ascontiguousarray(normals, "<f4").reshape(-1, 3)
        if normals.shape != verts.shape:
            raise ValueError("normals and vertices differ in shape")
        verts = np.concatenate([verts, normals], axis=1)
    if quality is not None:
        quality = np.ascontiguousarray(quality, "<f4").reshape(-1, 1)
        if len(quality) != len(verts):
            raise ValueError("quality and vertices differ in length")
        # (as words: a concatenation of floats may quieten a signalling NaN; the quality is carried bit for bit)
        verts = np.concatenate([verts.view("<u4"), quality.view("<u4")], axis=1)
    faces = np.empty(len(idx), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"] = 3
    faces["v"] = idx
    return header(len(verts), len(idx), normals is not None, quality is not None) + verts.tobytes() + faces.tobytes()


def write_ply(path, verts, idx, normals=None, quality=None):
    with open(path, "wb") as f:
        f.write(ply_bytes(verts, idx, normals, quality))


def parse_ply(data, quality=False):
    """(verts (V, 3) float32, idx (F, 3) uint32, normals (V, 3) float32 or None) of a binary little-endian PLY whose vertices carry
    float x y z (nx ny nz) (quality) first and whose faces are triangles in a `list uchar int|uint` property. With quality=True a
    fourth value follows: the file's per-vertex quality (V,) float32, or None if it has none; without, a file that carries one is
    read all the same and the property is dropped."""
    data = bytes(data)
    end = data.find(b"end_header\n")
    if data[:4] != b"ply\n" or end < 0:
        raise ValueError("not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("only binary_little_endian 1.0 is read")
    elems, cur = [], None
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = [w[1], int(w[2]), []]
            elems.append(cur)
        elif w[:1] == ["property"] and cur is not None:
            cur[2].append(w[1:])
    if [e[0] for e in elems] != ["vertex", "face"]:
        raise ValueError("expected the elements vertex and face")
    (_, nv, vprops), (_, nf, fprops) = elems
    names = [p[1] for p in vprops]
    has_q = names[-1:] == ["quality"]
    if any(p[0] != "float" for p in vprops) or names[:len(names) - has_q] not in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]):
        raise ValueError("vertex properties must be float x y z (nx ny nz) (quality)")
    if len(fprops) != 1 or fprops[0][:2] != ["list", "uchar"] or fprops[0][2] not in ("int", "uint"):
        raise ValueError("faces must be one `list uchar int` property")
    off = end + len(b"end_header\n")
    stride = len(names)
    vb, fb = nv * stride * 4, nf * 13
    if len(data) != off + vb + fb:
        raise ValueError("file length does not match its header (triangles only)")
    v = np.frombuffer(data, "<f4", nv * stride, off).reshape(nv, stride)
    f = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<u4", (3,))]), nf, off + vb)
    if nf and (f["n"] != 3).any():
        raise ValueError("only triangles are read")
    out = (v[:, :3].copy(), f["v"].copy(), (v[:, 3:6].copy() if stride - has_q == 6 else None))
    return out + ((v[:, -1].copy() if has_q else None),) if quality else out


def read_ply(path, quality=False):
    with open(path, "rb") as f:
        return parse_ply(f.read(), quality)
