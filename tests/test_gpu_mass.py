"""gsdf_hip_indexed_mass and gsdf_hip_contour_sections on the device against the numpy / Python-integer twin of their contracts
(tests/massref.py): every float64 of every record, the raw sums and the derived values, equal BIT FOR BIT. The twin sees the mesh or
the loops and no device result. Shapes: the smallest at which each path of the kernels can go wrong (a partial wave, mixed waves,
uniform waves over two workgroups with a ragged tail, negative terms, the two ends of the exponent's range, faces that must be absent)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import massref as M
import toporef as T
from contourref import res_for
from scaffold.builder import Builder
from test_gpu_weld import records_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SPHERE_RESDIV = 10      # a welded unit sphere of about 300 faces (asserted below)
BOLT_RESDIV = 50        # the bolt with a few thousand faces (asserted below)


def same_records(got, want, what):
    """Two record arrays of one dtype, field by field (floats as bits), then as bytes."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in got.dtype.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        same = (a.view(np.uint64) == b.view(np.uint64)) if a.dtype.kind == "f" else (a == b)
        assert same.all(), (what, f, a[~same][:4], b[~same][:4])
    assert got.tobytes() == want.tobytes(), what


def check_mesh(gpu, v, i, what, ix=None):
    """Device records of (v, i) against the twin's; the report's bytes; a second call; returns (handle, total, shells, twin's integers)."""
    ix = ix or gpu.IndexedHIP.from_arrays(v, i)
    total, shells = ix.mass_records()
    assert total.dtype == M.MASS_DTYPE == gpu.MASS_DTYPE
    want_total, want_shells, ints = M.mesh_mass(v, i)
    print(what, "faces", len(i), "shells", len(shells), "e", int(total["exponent"]), "volume", float(total["volume"]), "second", total["second"].tolist(),
          "ms", ix.mass_ms())
    same_records(shells, want_shells, (what, "shells"))
    same_records(total, want_total, (what, "total"))
    rep, sh = ix.report(), ix.shells()
    assert total["label"] == M.TOTAL and (shells["label"] == sh["label"]).all() and total["exponent"] == rep.exponent
    assert np.float64(total["volume"]).tobytes() == np.float64(rep.volume).tobytes()
    assert total["centroid"].tobytes() == np.array(rep.centroid[:], np.float64).tobytes()
    assert shells["volume"].tobytes() == sh["volume"].tobytes() and shells["centroid"].tobytes() == sh["centroid"].tobytes()
    t2, s2 = ix.mass_records()
    assert t2.tobytes() == total.tobytes() and s2.tobytes() == shells.tobytes()      # computed once: the same bytes
    return ix, total, shells, ints


def sphere_mesh(gpu):
    shape = Builder().NewSphere(1)
    ix = records_mesh(gpu, gpu.SDF3HIP(shape), F32(float(shape.Diagonal()) / SPHERE_RESDIV), marched=False).weld()
    v, i, _ = ix.read()
    assert 256 < len(i) < 512 and len(i) % 64 != 0, len(i)         # two workgroups, a ragged last wave
    return ix, v, i


def test_tetrahedron_one_partial_wave(gpu):
    _, total, shells, _ = check_mesh(gpu, T.TET_V, T.TET_I, "tet")
    # corner at the origin, legs 6: volume 36, the integral of x^2 = 6^5 / 60, of x y = 6^5 / 120; e = 3, the contract's bound
    # n_tris 2^(5e-44) on the roundings of a term and its quantisation (tests/test_mass_ref.py derives it)
    assert total["volume"] == 36 and len(shells) == 1 and total["exponent"] == 3
    assert np.allclose(total["second"], [129.6, 129.6, 129.6, 64.8, 64.8, 64.8], rtol=0, atol=4 * 2.0 ** (5 * 3 - 44))


def test_two_cubes_with_alternating_faces_every_wave_mixed(gpu):
    (va, ia), (vb, ib) = M.box((1, 2, 3), (5, 6, 7)), M.box((-8, -8, -8), (-4, -6, -7))
    v = np.concatenate([va, vb])
    i = np.stack([ia, ib + np.uint32(8)], axis=1).reshape(-1, 3)            # a0 b0 a1 b1 ...
    ix, total, shells, ints = check_mesh(gpu, v, i, "two cubes")
    assert len(shells) == 2 and sorted(set(ix.shell_of()[1][:24:2].tolist())) == [0] and sorted(set(ix.shell_of()[1][1:24:2].tolist())) == [1]
    tot = [ints[0][k] + ints[1][k] for k in range(10)]
    same_records(total, M.mass_record(tot, int(total["exponent"]), M.TOTAL), "the total is the integer sum of the two shells")
    for s, (lo, hi) in zip(shells, (((1, 2, 3), (5, 6, 7)), ((-8, -8, -8), (-4, -6, -7)))):
        vol, first, second = M.box_moments(lo, hi)                          # e = 4: n_tris 2^(5e-44), the lower degrees far inside it
        atol = 12 * 2.0 ** (5 * 4 - 44)
        assert np.isclose(s["volume"], vol, rtol=0, atol=atol) and np.allclose(s["first"], first, rtol=0, atol=atol) and np.allclose(s["second"], second, rtol=0, atol=atol)


def test_sphere_uniform_waves_two_workgroups_and_its_inverse(gpu):
    ix, v, i = sphere_mesh(gpu)
    _, total, shells, ints = check_mesh(gpu, v, i, "sphere", ix)
    assert len(shells) == 1 and total["volume"] > 0 and (total["second"][:3] > 0).all()
    # inverted (b and c swapped): every q negative where it was positive (the signed high word). det is negated exactly, so the volume's
    # integer is; s_k and the bracket add in another order, so the other integers are the negatives up to those roundings: a few
    # 2^-53 of a term < 0.6 2^(5e), i.e. below 2^11 units of 2^(5e-62) per face
    _, t2, s2, ints2 = check_mesh(gpu, v, i[:, [0, 2, 1]].copy(), "sphere, inverted")
    assert ints2[0][0] == -ints[0][0] and all(abs(a + b) <= len(i) * 2 ** 11 for a, b in zip(ints[0], ints2[0]))
    assert t2["volume"] == -total["volume"] and (t2["second"][:3] < 0).all()
    # a sphere: three equal principal moments within what a coarse mesh gives, 2/5 m r^2 within 20 %
    tot, _ = ix.mass(density=2.0)
    assert tot["mass"] == 2.0 * tot["volume"] and np.allclose(tot["moments"], 0.4 * tot["mass"], rtol=0.2)
    assert np.allclose(tot["axes"] @ tot["axes"].T, np.eye(3), atol=1e-12) and np.linalg.det(tot["axes"]) > 0


@pytest.mark.parametrize("e", [128, -125])
def test_the_ends_of_the_exponent_range(gpu, e):
    _, v, i = sphere_mesh(gpu)
    scaled = (v.astype(np.float64) * 2.0 ** (e - T.exponent_of(v))).astype(np.float32)      # a power of two: the largest |coordinate| in [2^(e-1), 2^e)
    assert np.isfinite(scaled).all() and T.exponent_of(scaled) == e
    _, total, _, _ = check_mesh(gpu, scaled, i, "sphere at e = %d" % e)
    assert total["exponent"] == e and np.isfinite(total["second"]).all() and (total["second"][:3] > 0).all() and np.isfinite(total["inertia"]).all()


def test_degenerate_and_nonfinite_faces_are_absent(gpu):
    v = np.vstack([T.TET_V, [[np.nan, 1, 1]]]).astype(np.float32)
    i = np.vstack([T.TET_I, [[0, 0, 1]], [[1, 2, 4]]]).astype(np.uint32)
    ix, total, shells, _ = check_mesh(gpu, v, i, "tet + degenerate + NaN corner")
    rep = ix.report()
    assert rep.degenerate == 1 and rep.nonfinite == 1 and len(shells) == 1
    _, clean, _, _ = check_mesh(gpu, T.TET_V, T.TET_I, "tet")
    for f in ("volume", "first", "second", "centroid", "inertia"):
        assert np.ascontiguousarray(total[f]).tobytes() == np.ascontiguousarray(clean[f]).tobytes(), f


def test_bolt_welded_several_shells(gpu):
    shape = Builder().Scene("bolt")
    ix = records_mesh(gpu, gpu.SDF3HIP(shape), F32(float(shape.Diagonal()) / BOLT_RESDIV), marched=False).weld()
    v, i, _ = ix.read()
    assert 2000 < len(i) < 10000
    _, total, shells, _ = check_mesh(gpu, v, i, "bolt", ix)
    assert len(shells) >= 2 and total["volume"] > 0
    tot, per_shell = ix.mass(density=7.85)
    assert len(per_shell) == len(shells) and (np.diff(tot["moments"]) >= 0).all() and tot["moments"][0] > 0


def test_arguments_on_a_live_handle(gpu):
    L = gpu.lib()
    ix = gpu.IndexedHIP.from_arrays(*M.box((0, 0, 0), (1, 1, 1)))
    n, one, rec = C.c_uint64(99), np.zeros(1, M.MASS_DTYPE), np.zeros(1, M.MASS_DTYPE)
    assert L.gsdf_hip_indexed_mass(ix._h, None, None, 0, C.byref(n)) == 0 and n.value == 1
    assert L.gsdf_hip_indexed_mass(ix._h, None, None, 0, None) == -3 and L.gsdf_hip_indexed_mass(ix._h, None, rec.ctypes.data, 1, None) == -3
    n.value = 99
    assert L.gsdf_hip_indexed_mass(ix._h, one.ctypes.data, rec.ctypes.data, 0, C.byref(n)) == -9 and n.value == 1     # GSDF_ERR_SHORT_BUFFER
    assert L.gsdf_hip_indexed_mass(ix._h, one.ctypes.data, rec.ctypes.data, 1, C.byref(n)) == 0
    assert abs(one[0]["volume"] - 1) < 1e-12 and rec[0]["label"] == 0 and one[0]["label"] == M.TOTAL and np.allclose(one[0]["centroid"], 0.5, rtol=0, atol=1e-12)


# ---- sections ---------------------------------------------------------------------------------------------------------------------------
def check_sections(gpu, xy, loop_start, loop_layer, n_layers, what, dev=None):
    dev = dev or gpu.ContourHIP.from_arrays(xy, loop_start, loop_layer, n_layers)
    loops, layers = dev.sections()
    assert loops.dtype == M.SECTION_DTYPE == gpu.SECTION_DTYPE
    want_loops, want_layers, ints = M.sections(xy, loop_start, loop_layer, n_layers)
    print(what, "loops", len(loops), "verts", dev.n_verts, "layer 0", layers[0] if len(layers) else None, "ms", dev.sections_ms())
    same_records(loops, want_loops, (what, "loops"))
    same_records(layers, want_layers, (what, "layers"))
    ml, my = dev.measures()
    assert loops["area"].tobytes() == ml["area"].tobytes() and layers["area"].tobytes() == my["area"].tobytes()
    assert (loops["n_verts"] == ml["n_verts"]).all() and (loops["layer_or_n_loops"] == ml["layer"]).all()
    assert (layers["n_verts"] == my["n_verts"]).all() and (layers["layer_or_n_loops"] == my["n_loops"]).all()
    # each layer is its loops' integer sum
    layer = np.zeros(len(loops), np.int64) if loop_layer is None else np.asarray(loop_layer, np.int64)
    e = M.loop_exponent(xy)
    for l in range(n_layers):
        mine = np.flatnonzero(layer == l)
        tot = [sum(ints[q][k] for q in mine) for k in range(6)]
        same_records(layers[l], M.section_record(tot, e, int(loops["n_verts"][mine].sum()), len(mine)), (what, "layer", l))
    l2, y2 = dev.sections()
    assert l2.tobytes() == loops.tobytes() and y2.tobytes() == layers.tobytes()
    return loops, layers


def test_a_square(gpu):
    xy = np.array([[1, 2], [4, 2], [4, 6], [1, 6]], np.float32)
    loops, layers = check_sections(gpu, xy, [0, 4], None, 1, "square")
    s = loops[0]
    atol = 4 * 2.0 ** (4 * 3 - 44)       # e = 3: n 2^(4e-44), the roundings of a term and its quantisation; the first moments far inside it
    assert s["area"] == 12 and np.allclose(s["first"], [30, 48], rtol=0, atol=atol) and np.allclose(s["second"], [84, 208, 120], rtol=0, atol=atol)
    assert np.allclose(s["centroid"], [2.5, 4], rtol=0, atol=atol) and np.allclose(s["central"], [9, 16, 0], rtol=0, atol=64 * atol)
    assert layers[0].tobytes()[:88] == s.tobytes()[:88]


def test_two_hundred_small_loops_over_three_layers_mixed_waves(gpu):
    rng = np.random.default_rng(3)
    sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    parts = []
    for q in range(200):
        p = rng.integers(-40, 40, 2) + sq * rng.integers(1, 9, 2) * 0.25
        parts.append(p if q % 5 else p[::-1])                                # every fifth a hole (clockwise)
    xy = np.concatenate(parts).astype(np.float32)
    layer = np.sort(rng.integers(0, 3, 200)).astype(np.uint32)
    loops, layers = check_sections(gpu, xy, np.arange(201) * 4, layer, 3, "200 squares")
    assert (loops["area"][::5] < 0).all() and (loops["area"][1::5] > 0).all() and (layers["layer_or_n_loops"] > 0).all()


def test_one_loop_of_300_vertices_uniform_waves(gpu):
    t = np.arange(300) * (2 * np.pi / 300)
    xy = np.stack([3 + 2 * np.cos(t), -1 + 1.5 * np.sin(t)], axis=1).astype(np.float32)
    loops, _ = check_sections(gpu, xy, [0, 300], None, 1, "ellipse")
    # an ellipse a = 2, b = 1.5 about (3, -1): area pi a b, central xx = pi a^3 b / 4, yy = pi a b^3 / 4, within the polygon's 1e-3
    assert np.allclose(loops[0]["centroid"], [3, -1], atol=1e-6)
    assert np.allclose(loops[0]["central"], [np.pi * 8 * 1.5 / 4, np.pi * 2 * 1.5 ** 3 / 4, 0], rtol=1e-3, atol=1e-6)


def test_text_outline_simplified(gpu):
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sdf = gpu.SDF2HIP(mod.scene("text"))
    res = res_for(sdf.Bounds(), 150)
    dev, _ = gpu.ContourHIP.outline(sdf, res).simplify(F32(res / F32(8)), passes=2)
    assert dev.n_loops > 4 and dev.n_verts > 192                     # several loops inside one wave, more than three waves
    loops, layers = check_sections(gpu, dev.xy, dev.loop_start, dev.loop_layer, dev.n_layers, "text", dev)
    assert (loops["area"] < 0).any() and layers[0]["area"] > 0       # letters with holes; the layer is the material


def test_no_loops(gpu):
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F32(0.1))
    loops, layers = dev.sections()
    assert len(loops) == 0 and layers[0]["area"] == 0 and layers[0]["layer_or_n_loops"] == 0
    assert layers[0]["centroid"].view(np.uint64).tolist() == [0x7ff8000000000000] * 2 and layers[0]["central"].view(np.uint64).tolist() == [0x7ff8000000000000] * 3


# ---- the examples -----------------------------------------------------------------------------------------------------------------------
def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_print_mass_and_section_properties(gpu, tmp_path, capsys):
    import re
    assert _example("render_ply").main(["bolt", "--resdiv", str(BOLT_RESDIV), "--interpreter", "--report", "--density", "7.85", "-o", str(tmp_path / "bolt.ply")]) == 0
    said = capsys.readouterr().out
    m = re.search(r"^bolt mass: mass (\S+) \(volume (\S+) at density 7\.85\), centre \((\S+), (\S+), (\S+)\); inertia about it xx (\S+) .*; principal moments (\S+) (\S+) (\S+) about ", said, re.M)
    assert m, said
    mass, vol = float(m.group(1)), float(m.group(2))
    assert vol > 0 and abs(mass / (7.85 * vol) - 1) < 1e-8 and float(m.group(7)) <= float(m.group(8)) <= float(m.group(9))
    assert re.search(r"volume %s[, ]" % re.escape(m.group(2)), said.split("bolt mass:")[0])       # the report's volume, printed alike
    assert "  shell 0 (label 0): mass " in said and "  shell 1 (label " in said
    assert _example("render_svg").main(["text", "--resdiv", "120", "--interpreter", "--report", "-o", str(tmp_path / "text.svg")]) == 0
    said = capsys.readouterr().out
    m = re.search(r"^layer 0 section: area (\S+), centroid \((\S+), (\S+)\), second moments about it xx (\S+) yy (\S+) xy (\S+) ", said, re.M)
    assert m and float(m.group(1)) > 0 and float(m.group(4)) > 0 and float(m.group(5)) > 0, said
