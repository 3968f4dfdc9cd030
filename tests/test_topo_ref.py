"""The numpy twin of the report contract (tests/toporef.py) on meshes with known answers, against tests/weldref.py's edge check and
against closed forms -- and the library's side of the ABI (no GPU here).

Closed forms. Relative deviation of the twin's volume / area of the welded marching-cubes mesh from the solid's, measured here at
resdiv 60 -> 120 (a chord error: second order in the cell size, so the ratio is close to 4):
  sphere r = 1             volume 1.98e-3 -> 4.94e-4   area 1.04e-3 -> 2.61e-4
  torus R = 1, r = 0.47    volume 4.48e-3 -> 1.12e-3   area 1.38e-3 -> 3.44e-4
  two-spheres (1, 0.7)     volume 6.28e-3 -> 1.57e-3   area 3.52e-3 -> 8.80e-4; its shells at 60: volume 4.97e-3 (r = 1), 1.01e-2 (r = 0.7)
Asserted: the deviation at 120 below half of that at 60, and each deviation at 60 below twice the value above (CLOSED_FORM).

Example parts at resdiv 200 (EXAMPLE_SHELLS), from the twin: npt-flange, knurled-cylinder and glyph-plate are one shell each (the
flange and the knurled cylinder have one through hole: Euler 0). bolt is TWO shells of Euler 2 each, which is where
MANIFOLD_SCENES' Euler characteristic 4 comes from: the bolt itself and a speck of 14 vertices / 24 faces with positive volume (a
closed blob the thread's distance field leaves beside it), what `--min-shell-tris` is for. fibonacci-showerhead is ONE shell of
Euler -258 = 2 - 2 * 130: a single solid of genus 130, the spray holes being through holes of one body, not separate shells."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import toporef as T
import weldref as W
from test_weld_ref import MANIFOLD_SCENES, twin_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
# scene -> (volume, area, twice the measured relative deviation of volume and of area at resdiv 60)
CLOSED_FORM = {
    "sphere": (4 * PI / 3, 4 * PI, 4.0e-3, 2.1e-3),
    "torus": (2 * PI * PI * 0.47 ** 2, 4 * PI * PI * 0.47, 9.0e-3, 2.8e-3),
    "two-spheres": (4 * PI / 3 * (1 + 0.7 ** 3), 4 * PI * (1 + 0.7 ** 2), 1.26e-2, 7.1e-3),
}
# scene -> per shell (n_verts, n_tris, euler, sign of volume), resdiv 200
EXAMPLE_SHELLS = {
    "npt-flange": [(52716, 105432, 0, 1)],
    "bolt": [(31074, 62144, 2, 1), (14, 24, 2, 1)],
    "knurled-cylinder": [(98166, 196332, 0, 1)],
    "glyph-plate": [(29680, 59356, 2, 1)],
    "fibonacci-showerhead": [(49160, 98836, -258, 1)],
}
_cache = {}


def analysed(name, resdiv):
    if (name, resdiv) not in _cache:
        _, _, v, idx, _, _ = twin_of(name, resdiv)
        _cache[(name, resdiv)] = (v, idx, T.analyse(v, idx))
    return _cache[(name, resdiv)]


@pytest.mark.parametrize("name,resdiv,expect", MANIFOLD_SCENES)
def test_twin_agrees_with_edge_report(name, resdiv, expect):
    v, idx, tw = analysed(name, resdiv)
    rep, er = tw["report"], W.edge_report(idx)
    assert bool(rep["closed_oriented"]) == er["closed_oriented"] is True
    assert (rep["used_verts"], rep["n_tris"], rep["euler"]) == (er["V"], er["F"], er["euler"]) == expect
    assert rep["edges"] == er["E"] and rep["degenerate"] == er["degenerate"] == 0 and rep["nonfinite"] == 0
    sh = tw["shells"]
    assert sh["euler"].sum() == rep["euler"] and sh["n_verts"].sum() == rep["used_verts"] and sh["n_tris"].sum() == rep["n_tris"]
    if name in EXAMPLE_SHELLS:
        got = [(int(s["n_verts"]), int(s["n_tris"]), int(s["euler"]), int(np.sign(s["volume"]))) for s in sh]
        assert got == EXAMPLE_SHELLS[name]


def test_edge_report_flags_agree_on_damaged_meshes():
    for name, (v, i) in T.hand_meshes().items():
        assert bool(T.analyse(v, i)["report"]["closed_oriented"]) == W.edge_report(i)["closed_oriented"], name


def test_hand_meshes():
    hm = T.hand_meshes()
    r = T.analyse(*hm["tet"])
    rep, sh = r["report"], r["shells"]
    assert (rep["n_shells"], rep["euler"], rep["edges"], rep["closed_oriented"], rep["exponent"]) == (1, 2, 6, 1, 3)
    assert rep["volume"] == 36.0 and (rep["centroid"] == 1.5).all()                      # exact: every term is an integer
    assert abs(rep["area"] - (54 + 18 * math.sqrt(3))) < 1e-12
    assert (rep["bbox"] == [0, 0, 0, 6, 6, 6]).all() and sh["label"][0] == 0 and sh.tobytes() == T.analyse(*hm["tet"])["shells"].tobytes()
    assert (r["shell_of_vertex"] == 0).all() and (r["shell_of_face"] == 0).all()
    rep = T.analyse(*hm["tet-hole"])["report"]
    assert (rep["boundary_edges"], rep["misoriented_edges"], rep["nonmanifold_edges"], rep["closed_oriented"], rep["euler"]) == (3, 0, 0, 0, 1)
    rep = T.analyse(*hm["tet-flipped"])["report"]
    assert (rep["boundary_edges"], rep["misoriented_edges"], rep["nonmanifold_edges"], rep["closed_oriented"], rep["euler"]) == (0, 3, 0, 0, 2)
    r = T.analyse(*hm["tet-degenerate"])
    rep = r["report"]
    assert (rep["degenerate"], rep["closed_oriented"], rep["euler"], rep["volume"], rep["edges"]) == (1, 0, 2, 36.0, 6)
    assert r["shell_of_face"][-1] == T.NONE
    r = T.analyse(*hm["two-tets-one-edge"])
    rep = r["report"]
    assert (rep["nonmanifold_edges"], rep["n_shells"], rep["boundary_edges"], rep["misoriented_edges"], rep["volume"]) == (1, 1, 0, 0, 72.0)
    r = T.analyse(*hm["two-tets-apart"])
    rep, sh = r["report"], r["shells"]
    assert (rep["n_shells"], rep["euler"], rep["closed_oriented"], rep["exponent"]) == (2, 4, 1, 5)
    assert list(sh["label"]) == [0, 4] and list(sh["volume"]) == [36.0, 36.0] and rep["volume"] == 72.0
    assert (sh["centroid"] == [[1.5] * 3, [19.5] * 3]).all() and (sh["bbox"][1] == [18, 18, 18, 24, 24, 24]).all()
    r = T.analyse(*hm["cube-in-cube"])
    rep, sh = r["report"], r["shells"]
    assert (rep["n_shells"], rep["closed_oriented"], rep["euler"]) == (2, 1, 4)
    assert list(sh["volume"]) == [13824.0, -1728.0] and rep["volume"] == 12096.0 and list(sh["area"]) == [3456.0, 864.0] and rep["area"] == 4320.0
    assert (sh["centroid"] == 12.0).all() and (rep["centroid"] == 12.0).all()
    r = T.analyse(*hm["tet-nan"])
    rep = r["report"]
    assert (rep["nonfinite"], rep["closed_oriented"], rep["n_shells"], rep["euler"]) == (3, 1, 1, 2)   # topology counts them, the measures do not
    assert rep["volume"] == 0.0 and rep["area"] == 18.0 and np.isnan(rep["centroid"]).all()           # the face left: (0, 2, 1), in z = 0
    assert (rep["bbox"] == [0, 0, 0, 6, 6, 0]).all()
    # a mesh whose every face is degenerate: no shells, an empty box
    rep = T.analyse(T.TET_V, np.array([[0, 0, 1]]))["report"]
    assert rep["n_shells"] == 0 and rep["used_verts"] == 0 and rep["bbox"][0] == np.inf and rep["bbox"][3] == -np.inf


@pytest.mark.parametrize("name", sorted(CLOSED_FORM))
def test_closed_forms_and_convergence(name):
    vol, area, bound_v, bound_a = CLOSED_FORM[name]
    dev = {}
    for resdiv in (60, 120):
        rep = analysed(name, resdiv)[2]["report"]
        dev[resdiv] = (abs(rep["volume"] - vol) / vol, abs(rep["area"] - area) / area)
        print(name, resdiv, "relative deviation of volume, area:", dev[resdiv])
    assert dev[60][0] <= bound_v and dev[60][1] <= bound_a
    assert dev[120][0] < 0.5 * dev[60][0] and dev[120][1] < 0.5 * dev[60][1]
    r = analysed(name, 60)[2]
    if name == "torus":
        assert r["report"]["n_shells"] == 1 and r["report"]["euler"] == 0
    if name == "two-spheres":
        sh = r["shells"]
        assert len(sh) == 2 and list(sh["euler"]) == [2, 2]
        d0 = abs(sh["volume"][0] - 4 * PI / 3) / (4 * PI / 3)
        d1 = abs(sh["volume"][1] - 4 * PI / 3 * 0.343) / (4 * PI / 3 * 0.343)
        print("shells:", d0, d1)
        assert d0 <= 1.0e-2 and d1 <= 2.02e-2                                           # twice 4.97e-3, 1.01e-2
        assert np.abs(sh["centroid"][0] - [-1.5, 0, 0]).max() < 1e-3 and np.abs(sh["centroid"][1] - [1.5, 0.1, 0.2]).max() < 1e-3


def test_order_independence():
    for v, i in (T.random_soup(), analysed("two-spheres", 60)[:2]):
        a = T.analyse(v, i)
        perm = np.random.default_rng(1).permutation(len(i))
        b = T.analyse(v, np.asarray(i)[perm])
        ra, rb = a["report"], b["report"]
        for k in ra:
            x, y = np.asarray(ra[k]), np.asarray(rb[k])
            assert x.tobytes() == y.tobytes(), k
        assert a["shells"].tobytes() == b["shells"].tobytes()
        assert (a["shell_of_vertex"] == b["shell_of_vertex"]).all() and (a["shell_of_face"][perm] == b["shell_of_face"]).all()
    # ... and of the vertex numbering, the labels mapped through it: the integer counts and the measures' bits per shell
    v, i = analysed("two-spheres", 60)[:2]
    a = T.analyse(v, i)
    vp = np.random.default_rng(2).permutation(len(v))      # new number of old vertex k: vp[k]
    v2 = np.empty_like(v)
    v2[vp] = v
    b = T.analyse(v2, vp[np.asarray(i).astype(np.int64)])
    assert a["report"]["volume"].tobytes() == b["report"]["volume"].tobytes() and a["report"]["area"].tobytes() == b["report"]["area"].tobytes()
    mapped = b["shell_of_vertex"][vp]                       # shell of old vertex k in the renumbered mesh
    order = [int(mapped[a["shell_of_vertex"] == s][0]) for s in range(2)]
    for f in ("n_verts", "n_tris", "edges", "euler", "area", "volume", "centroid", "bbox"):
        assert a["shells"][f].tobytes() == b["shells"][f][order].tobytes(), f
    assert [int(b["shells"]["label"][o]) for o in order] == [int(vp[a["shell_of_vertex"] == s].min()) for s in range(2)]


def test_random_soup_is_what_the_gpu_test_needs():
    v, i = T.random_soup()
    rep = T.analyse(v, i)["report"]
    assert len(v) == 5000 and len(i) == 20000 and rep["n_shells"] > 200
    assert min(rep["degenerate"], rep["nonfinite"], rep["boundary_edges"], rep["nonmanifold_edges"], rep["misoriented_edges"]) > 0


def test_extract_twin():
    v, i = T.hand_meshes()["cube-in-cube"]
    r = T.analyse(v, i)
    keys = np.arange(len(v), dtype=np.uint64) + np.uint64(100)
    v2, i2, k2, _ = T.extract(v, i, keys, None, r["shell_of_face"], [False, True])
    assert len(v2) == 8 and len(i2) == 12 and (k2 >= 108).all()
    flat = i2.reshape(-1).astype(np.int64)
    uniq, first = np.unique(flat, return_index=True)
    assert (uniq == np.arange(8)).all() and (np.diff(first) > 0).all()       # numbered by first appearance
    rep = T.analyse(v2, i2)["report"]
    assert rep["volume"] == -1728.0 and rep["closed_oriented"] == 1


def test_abi_symbols_and_struct_sizes():
    """The library exports the report's entry points, and the ctypes / numpy mirrors are as large as the header asserts."""
    from gsdf_amd import hip
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    L = hip.lib()
    for name in ("gsdf_hip_indexed_create", "gsdf_hip_indexed_report", "gsdf_hip_indexed_shells", "gsdf_hip_indexed_read_shell_of", "gsdf_hip_indexed_extract"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name) and name in hip.SYMBOLS, name
    size = lambda t: int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, hdr).group(1))
    assert C.sizeof(hip.IndexedReport) == size("gsdf_indexed_report") == 208
    assert hip.SHELL_DTYPE.itemsize == T.SHELL_DTYPE.itemsize == size("gsdf_shell") == 136 and hip.SHELL_DTYPE == T.SHELL_DTYPE
    for f, off in (("degenerate", 16), ("edges", 40), ("n_shells", 72), ("euler", 80), ("area", 88), ("centroid", 104), ("bbox", 128), ("closed_oriented", 152),
                   ("exponent", 156), ("ms_edges", 160), ("probes", 184), ("attempts", 200)):
        assert getattr(hip.IndexedReport, f).offset == off and re.search(r"offsetof\(gsdf_indexed_report, %s\) == %d\b" % (f, off), hdr), f
    assert hip.IndexedReport.RESULT_BYTES == hip.IndexedReport.ms_edges.offset
    for f, off in (("nonfinite", 16), ("edges", 24), ("euler", 56), ("area", 64), ("centroid", 80), ("bbox", 104), ("label", 128)):
        assert hip.SHELL_DTYPE.fields[f][1] == off and re.search(r"offsetof\(gsdf_shell, %s\) == %d\b" % (f, off), hdr), f
    # host-side argument checks need no device
    h = C.c_void_p()
    v, i = T.hand_meshes()["tet"]
    assert L.gsdf_hip_indexed_create(v.ctypes.data, 0, i.ctypes.data, 4, None, C.byref(h)) == -1     # GSDF_ERR_EMPTY_BUFFERS
    bad = i.copy()
    bad[2, 0] = 9
    assert L.gsdf_hip_indexed_create(v.ctypes.data, 4, bad.ctypes.data, 4, None, C.byref(h)) == -3 and not h.value
    msg = L.gsdf_hip_last_error().decode()
    assert "face 2" in msg and "index 9" in msg
    assert L.gsdf_hip_indexed_report(None, None) == -3
