"""A numpy twin of the indexed-mesh CLEAN contract (include/gsdf_hip.h, "indexed meshes: clean"), written from the header text alone:
(verts, idx, keys, normals, flags) in; the cleaned mesh and the stats' leading block out. Nothing here looks at a device result.

Classes by np.unique over the rows of canonical position words (non-finite vertices get a row of their own), sets by np.unique over
the sorted index triples, the result's numbering by first appearance as in toporef.extract."""
import struct

import numpy as np

MERGE_POSITIONS, FACES = 1, 2
# the leading block of gsdf_clean_stats, in its order: eleven uint64 (88 bytes)
STAT_FIELDS = ["n_verts_in", "n_tris_in", "merged_verts", "degenerate", "face_sets", "cancelled_sets", "duplicate_faces", "opposite_faces",
               "largest_set", "n_verts", "n_tris"]
BAD_ARGUMENT, EMPTY_BUFFERS = -3, -1


class CleanError(Exception):
    """code: the GSDF_ERR_* the device returns for the same input."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code
        self.msg = msg


def stats_bytes(st):
    return struct.pack("<11Q", *[int(st[f]) for f in STAT_FIELDS])


def classes(verts, flags):
    """Step 1: (V,) int64, every vertex's class = the smallest vertex number with its position key."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    own = np.arange(len(v), dtype=np.int64)
    if not flags & MERGE_POSITIONS or len(v) == 0:
        return own
    w = v.view(np.uint32).astype(np.uint64)
    w = np.where(w == 0x80000000, 0, w)
    finite = ((w & 0x7fffffff) < 0x7f800000).all(axis=1)
    rows = np.concatenate([w, np.zeros((len(v), 1), np.uint64)], axis=1)
    rows[~finite] = 0
    rows[~finite, 3] = own[~finite].astype(np.uint64) + 1       # a row of its own (the fourth word of a finite vertex is 0)
    _, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    smallest = np.full(inv.max() + 1, len(v), np.int64)
    np.minimum.at(smallest, inv, own)
    return smallest[inv]


def orientation(faces):
    """Step 3, per non-degenerate face (n, 3) int64: (sorted triples (n, 3), minus (n,) bool)."""
    s = np.sort(faces, axis=1)
    at = np.argmin(faces, axis=1)
    nxt = faces[np.arange(len(faces)), (at + 1) % 3]
    return s, nxt != s[:, 1]


def clean(verts, idx, keys, normals, flags, dry=False):
    """(verts (V2, 3) float32, idx (F2, 3) uint32, keys (V2,) uint64, normals (V2, 3) float32 or None, stats dict). dry: (None, None,
    None, None, stats), and no error where nothing is kept. keys None: zeros, as an upload without keys reads back."""
    flags = int(flags)
    if flags == 0 or flags & ~(MERGE_POSITIONS | FACES):
        raise CleanError(BAD_ARGUMENT, "flags")
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    k = np.zeros(len(v), np.uint64) if keys is None else np.asarray(keys, np.uint64).reshape(-1)
    cls = classes(v, flags)
    m = cls[i]
    deg = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2])
    keep = ~deg
    st = {"n_verts_in": len(v), "n_tris_in": len(i), "merged_verts": int((cls != np.arange(len(v))).sum()), "degenerate": int(deg.sum()),
          "face_sets": 0, "cancelled_sets": 0, "duplicate_faces": 0, "opposite_faces": 0, "largest_set": 0}
    if flags & FACES and keep.any():
        nd = np.flatnonzero(keep)
        sets, minus = orientation(m[nd])
        _, inv = np.unique(sets, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n = inv.max() + 1
        f = np.bincount(inv[~minus], minlength=n)
        r = np.bincount(inv[minus], minlength=n)
        first = np.full((n, 2), len(i), np.int64)               # the smallest face number per set and orientation
        np.minimum.at(first, (inv, minus.astype(np.int64)), nd)
        major = (r > f).astype(np.int64)
        winner = np.where(f != r, first[np.arange(n), major], -1)
        keep[nd] = winner[inv] == nd
        st.update(face_sets=int(n), cancelled_sets=int((f == r).sum()), opposite_faces=int(2 * np.minimum(f, r).sum()),
                  duplicate_faces=int((np.abs(f - r) - 1)[f != r].sum()), largest_set=int((f + r).max()))
    kept = m[keep]
    flat = kept.reshape(-1)
    uniq, first_slot, finv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first_slot, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    old = uniq[order]
    st.update(n_verts=len(uniq), n_tris=len(kept))
    if dry:
        return None, None, None, None, st
    if len(kept) == 0:
        raise CleanError(EMPTY_BUFFERS, "nothing kept")
    return (v[old].copy(), number[finv.reshape(-1)].reshape(-1, 3).astype(np.uint32), k[old].copy(),
            None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)[old].copy(), st)
