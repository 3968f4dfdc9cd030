"""The numpy twin of the indexed-mesh contract (tests/weldref.py) against the oracle's octree renderer, the edge check that the GPU
tests rely on, the PLY reader and writer -- and the choice of the scenes the GPU manifold test runs (no GPU here).

Scenes. The twin was run over the five example parts at resdiv 200 and over a sphere, a torus and two disjoint spheres at resdiv
60. Under the reference's marching-cubes table (Bourke's, which may legitimately share an edge among four triangles on an ambiguous
face, and which gives degenerate triangles at an exactly-zero corner) ALL of them came out as closed oriented manifolds with no
degenerate triangle, so all of them are in MANIFOLD_SCENES with the counts measured then. npt-flange at resdiv 400 (the GPU
contract test's scene) likewise: V = 211 926, F = 423 852, Euler 0.

Position bound. A slot that does not own its vertex may differ from it by at most res / 64 per coordinate ("same lattice edge",
a condition, not a measurement). The largest difference observed in the oracle's soup over these scenes, in units of res:
sphere 1.8e-5, torus 4.3e-5, two-spheres 3.3e-5, npt-flange 1.1e-4 (resdiv 400: 2.0e-3), bolt 5.4e-4, knurled-cylinder 1.1e-3,
glyph-plate 7.4e-5, fibonacci-showerhead 4.3e-3 -- all below 1 / 64 = 1.6e-2; asserted below for every scene."""
import numpy as np
import pytest

import weldref as W
from gsdf_amd import ply
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

POSITION_BOUND_DIV = 64

# (scene, resdiv, (V, F, V - E + F)) as the twin gives them; every one a closed oriented manifold
MANIFOLD_SCENES = [
    ("sphere", 60, (5616, 11228, 2)),
    ("torus", 60, (5260, 10520, 0)),
    ("two-spheres", 60, (3330, 6652, 4)),
    ("npt-flange", 200, (52716, 105432, 0)),
    ("bolt", 200, (31088, 62168, 4)),
    ("knurled-cylinder", 200, (98166, 196332, 0)),
    ("glyph-plate", 200, (29680, 59356, 2)),
    ("fibonacci-showerhead", 200, (49160, 98836, -258)),
]


def scene_shape(b, name):
    if name == "sphere":
        return b.NewSphere(1)
    if name == "torus":
        return b.NewTorus(1.0, 0.47)
    if name == "two-spheres":
        return b.Union(b.Translate(b.NewSphere(1), -1.5, 0, 0), b.Translate(b.NewSphere(0.7), 1.5, 0.1, 0.2))
    return b.Scene(name)


def twin_of(name, resdiv):
    shape = scene_shape(Builder(), name)
    cpu = OracleSDF(shape.tree())
    res = np.float32(float(shape.Diagonal()) / resdiv)
    origin, levels = W.lattice_of(shape.Bounds(), res)
    ref = cpu.render_octree(res)
    assert levels == ref.levels
    leaves = W.leaves_of_triangles(ref.tris, origin, res)
    v, i, k, soup = W.weld(cpu, leaves, origin, res)
    return res, ref, v, i, k, soup


@pytest.mark.parametrize("name,resdiv,expect", MANIFOLD_SCENES)
def test_twin_against_oracle_and_edge_check(name, resdiv, expect):
    res, ref, v, idx, keys, soup = twin_of(name, resdiv)
    bound = float(res) / POSITION_BOUND_DIV
    # the twin's de-indexed triangles are the oracle's, as a sorted set, within the position bound (its soup: bit for bit)
    a, b = W.sorted_triangles(soup), W.sorted_triangles(ref.tris)
    assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()
    deidx = v[idx.reshape(-1)]
    worst = float(np.abs(deidx.astype(np.float64) - soup.astype(np.float64)).max())
    assert worst <= bound, (worst / float(res))
    # (sorted by the soup's own order: sorting the welded copies independently could swap rows that differ in their last bits)
    s9 = soup.reshape(-1, 9)
    c = deidx.reshape(-1, 9)[np.lexsort(s9.T[::-1])]
    assert c.shape == b.shape and float(np.abs(c.astype(np.float64) - b.astype(np.float64)).max()) <= bound
    # the contract's numbering: owners in slot order, their positions the soup's bits
    flat = idx.reshape(-1).astype(np.int64)
    uniq, first = np.unique(flat, return_index=True)
    assert (uniq == np.arange(len(v))).all() and (np.diff(first) > 0).all()
    assert (v.view(np.uint32) == soup[first].view(np.uint32)).all() and len(np.unique(keys)) == len(keys) == len(v)
    rep = W.edge_report(idx)
    assert rep["closed_oriented"] and rep["degenerate"] == 0, rep
    assert (rep["V"], rep["F"], rep["euler"]) == expect, rep
    # a bitwise weld of the same soup leaves cracks: the check discriminates
    _, inv = np.unique(soup.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    assert not W.edge_report(inv.reshape(-1, 3))["closed_oriented"]


def test_edge_report_on_known_meshes():
    tet = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    rep = W.edge_report(tet)
    assert rep["closed_oriented"] and rep["euler"] == 2
    assert not W.edge_report(tet[:3])["closed_oriented"]                       # a hole
    flipped = tet.copy()
    flipped[0] = flipped[0][::-1]
    assert not W.edge_report(flipped)["closed_oriented"]                       # one face wound the other way
    assert not W.edge_report(np.vstack([tet, [[0, 0, 1]]]))["closed_oriented"]  # a degenerate face


def test_key_packing():
    k = W.pack_key(np.array([[1, 2, 3], [65536, 65536, 65536]]), np.array([2, 3]))
    assert int(k[0]) == 1 | (2 << 20) | (3 << 40) | (2 << 60) and int(k[1]) >> 60 == 3 and (int(k[1]) >> 40) & 0xfffff == 65536


def test_ply_round_trip(tmp_path):
    _, _, v, idx, _, _ = twin_of("torus", 30)
    rng = np.random.default_rng(3)
    nrm = rng.standard_normal(v.shape).astype(np.float32)
    nrm[0, 0] = np.nan
    for normals in (None, nrm):
        data = ply.ply_bytes(v, idx, normals)
        hdr = ply.header(len(v), len(idx), normals is not None)
        assert data.startswith(hdr) and len(hdr) % 4 == 0 and len(data) == len(hdr) + len(v) * (24 if normals is not None else 12) + 13 * len(idx)
        assert b"format binary_little_endian 1.0\n" in hdr and f"element vertex {len(v)}\n".encode() in hdr
        assert b"property list uchar int vertex_indices\n" in hdr and hdr.endswith(b"end_header\n")
        p = tmp_path / "t.ply"
        ply.write_ply(p, v, idx, normals)
        v2, i2, n2 = ply.read_ply(p)
        assert (v2.view(np.uint32) == v.view(np.uint32)).all() and (i2 == idx).all()
        assert (n2 is None) if normals is None else (n2.view(np.uint32) == nrm.view(np.uint32)).all()
    for v_count in range(1, 12):   # the padding keeps every header a multiple of four bytes long
        assert len(ply.header(10 ** v_count, 7)) % 4 == 0
    with pytest.raises(ValueError):
        ply.parse_ply(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        ply.parse_ply(ply.ply_bytes(v, idx)[:-1])
    with pytest.raises(ValueError):
        ply.ply_bytes(v, idx + len(v))
