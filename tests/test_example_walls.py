"""Walls through examples/render_svg.py and gsdf_amd/svg.py: on the host alone, write_svg(..., walls=...) keeps the layers' loops
readable bit for bit and read_svg_walls returns the twin's offset loops; on the device, the example's file holds the walls of
ContourHIP.offset at (i + 0.5) W res and the hatch of the loops at N W res, which are the twins' for the traced loops."""
import importlib.util
import os
import re

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
import offsetref as O
from gsdf_amd import svg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wall_insets(n, width, res):
    """The example's insets, in its float32 arithmetic: the walls' middles and the inner edge of the stack."""
    w = F(F(width) * res)
    return [F(F(i + 0.5) * w) for i in range(n)], F(F(n) * w)


def test_write_svg_with_walls_round_trips_loops_and_walls(tmp_path):
    c = H.hand_loops()
    o = O.offset(c, 0.25, (0.25, 0.75))
    layers = [[l for l, q in zip(c.loops(), c.loop_layer) if q == k] for k in range(c.n_layers)]
    walls = [[o.loops(2 * k + i) for i in range(2)] for k in range(c.n_layers)]
    h = H.hatch(S.Loops.of(O.offset(c, 0.25, (1.0,))), 0.5, H.directions((45.0, 135.0)))
    plain, walled = str(tmp_path / "a.svg"), str(tmp_path / "b.svg")
    svg.write_svg(plain, layers, hatch=[h.segments(k) for k in range(c.n_layers)])
    svg.write_svg(walled, layers, hatch=[h.segments(k) for k in range(c.n_layers)], walls=walls)
    a, b = svg.read_svg(plain), svg.read_svg(walled)
    assert len(a) == len(b) == c.n_layers
    for la, lb, want in zip(a, b, layers):
        assert [x.tobytes() for x in la] == [x.tobytes() for x in lb] == [np.asarray(w, F).tobytes() for w in want]
    text = open(walled).read()
    assert text.count('<path class="wall"') == 2 * c.n_layers and "wall" not in open(plain).read()
    assert text.count("<path ") == 3 * c.n_layers
    assert np.concatenate(svg.read_svg_hatch(walled)).tobytes() == h.seg.tobytes()
    back = svg.read_svg_walls(walled)
    assert len(back) == c.n_layers and all(len(w) == 2 for w in back) and svg.read_svg_walls(plain) == []
    for got, want in zip(back, walls):
        for gl, wl in zip(got, want):
            assert [x.tobytes() for x in gl] == [np.asarray(x, F).tobytes() for x in wl]
    assert back[3] == [[], []] and len(back[0][0]) == 2   # the empty layer; an annulus keeps its two loops


def _check_file(gpu, ex, out, said, c, res, n, width, hatch, angles):
    """The file's walls and hatch against the twins for the traced loops `c`."""
    insets, edge = wall_insets(n, width, res)
    ref = S.Loops.of(c)
    want = O.offset(ref, res, insets)
    back = svg.read_svg_walls(str(out))
    assert len(back) == c.n_layers and all(len(w) == n for w in back)
    for k in range(c.n_layers):
        for i in range(n):
            assert [x.tobytes() for x in back[k][i]] == [x.tobytes() for x in want.loops(k * n + i)], (k, i)
    layers = svg.read_svg(str(out))
    assert len(layers) == c.n_layers and np.concatenate([l for ls in layers for l in ls]).tobytes() == c.xy.tobytes()
    fill = O.offset(ref, res, [edge])
    wh = H.hatch(S.Loops.of(fill), F(F(hatch) * res), H.directions(angles))
    assert np.concatenate(svg.read_svg_hatch(str(out))).tobytes() == wh.seg.tobytes() and wh.stats["n_segments"] > 0
    # the report: every layer's walls, their lengths those of the twin's measures; the two offsets' costs
    _, meas = S.measures(S.Loops.of(want))
    rows = re.findall(r"layer (\d+) walls: length (.*?) = (\S+) \((\d+) loops\)", said)
    assert [int(r[0]) for r in rows] == list(range(c.n_layers)), said
    for k, r in enumerate(rows):
        assert [float(v) for v in r[1].split(" + ")] == [float("%.9g" % meas[k * n + i]["length"]) for i in range(n)]
        assert int(r[3]) == sum(int(meas[k * n + i]["n_loops"]) for i in range(n))
    m = re.search(r"walls: %d inset\(s\).*?device time (\S+) ms = distance field (\S+) \+ tracing (\S+)" % n, said)
    assert m and float(m.group(2)) > 0 and float(m.group(3)) > 0 and "fill boundary: 1 inset(s)" in said, said


@pytest.mark.gpu
def test_render_svg_text_with_walls(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "text.svg"
    assert ex.main(["text", "--resdiv", "200", "--interpreter", "--walls", "2", "--wall-width", "0.75", "--hatch", "1", "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    sdf = gpu.SDF2HIP(ex.scene("text"))
    res = ex.spacing(sdf.Bounds(), False, 200.0)
    _check_file(gpu, ex, out, said, ex.trace(gpu, sdf, res), res, 2, 0.75, 1, (45.0, 135.0))


@pytest.mark.gpu
def test_render_svg_bolt_with_walls_and_skin(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "bolt.svg"
    assert ex.main(["bolt", "--layer-height", "8", "--resdiv", "80", "--interpreter", "--walls", "3", "--wall-width", "1", "--hatch", "2", "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    sdf = gpu.SDF3HIP(ex.scene("bolt"))
    bb = sdf.Bounds()
    res = ex.spacing(bb, True, 80.0)
    c = ex.trace(gpu, sdf, res, gpu.layer_heights(bb, 8.0))
    assert c.n_layers >= 2
    _check_file(gpu, ex, out, said, c, res, 3, 1, 2, (45.0, 135.0))
    # with --skin the same walls, the pieces classed
    assert ex.main(["bolt", "--layer-height", "8", "--resdiv", "80", "--interpreter", "--walls", "3", "--wall-width", "1", "--hatch", "2", "--skin", "1", "1", "-o", str(out)]) == 0
    assert len(svg.read_svg_walls(str(out))) == c.n_layers and sum(len(q) for q in svg.read_svg_hatch_class(str(out))) > 0


def test_the_example_refuses_half_a_wall_option(capsys):
    ex = _example()
    for argv, why in ((["text", "--walls", "2"], "--walls N and --wall-width W go together"), (["text", "--wall-width", "2"], "--walls N and --wall-width W go together"),
                      (["text", "--walls", "9", "--wall-width", "1"], "--walls takes 1 .. 8 walls of a positive width"),
                      (["text", "--walls", "0", "--wall-width", "1"], "--walls takes 1 .. 8 walls of a positive width"),
                      (["text", "--walls", "2", "--wall-width", "0"], "--walls takes 1 .. 8 walls of a positive width")):
        with pytest.raises(SystemExit):
            ex.main(argv)
        assert why in capsys.readouterr().err, argv
