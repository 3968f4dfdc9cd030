"""Skin classes through examples/render_svg.py and gsdf_amd/svg.py: --skin writes the twin's pieces with the twin's classes and
reports the classes' areas and the overhangs; on the host alone, write_svg(..., hatch_class=...) round-trips loops, segments and
classes, and without hatch_class the file is byte for byte what the module wrote before classes existed."""
import importlib.util
import os
import re

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
import skinref as K
from gsdf_amd import svg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_write_svg_round_trips_the_classes(tmp_path):
    c = H.hand_loops()
    h = K.skin(c, 0.5, H.directions((45.0, 135.0)), 1, 1, 0.0437)
    assert set(h.cls.tolist()) == {0, 1, 2, 3}
    layers = [[l for l, q in zip(c.loops(), c.loop_layer) if q == k] for k in range(c.n_layers)]
    segs = [h.segments(k) for k in range(c.n_layers)]
    cls = [h.cls[h.layer_start[k]:h.layer_start[k + 1]] for k in range(c.n_layers)]
    plain, classed = str(tmp_path / "a.svg"), str(tmp_path / "b.svg")
    svg.write_svg(plain, layers, hatch=segs)
    svg.write_svg(classed, layers, hatch=segs, hatch_class=cls)
    for path in (plain, classed):
        back = svg.read_svg_hatch(path)
        assert len(back) == c.n_layers and np.concatenate(back).tobytes() == h.seg.tobytes()
        assert np.concatenate([np.concatenate(l) for l in svg.read_svg(path) if l]).tobytes() == c.xy.tobytes()
    back = svg.read_svg_hatch_class(classed)
    assert [len(b) for b in back] == np.diff(h.layer_start.astype(np.int64)).tolist() and np.concatenate(back).tobytes() == h.cls.tobytes()
    with pytest.raises(ValueError):
        svg.read_svg_hatch_class(plain)
    with pytest.raises(ValueError):
        svg.write_svg(classed, layers, hatch=segs, hatch_class=[k[:-1] for k in cls])
    # four strokes, one per class; without classes every line is the bare element of the plain hatch
    text = open(classed).read()
    assert [text.count('data-class="%d" stroke="%s"' % (q, svg.SKIN_STROKES[q])) for q in range(4)] == h.stats["n_class"] and len(set(svg.SKIN_STROKES)) == 4
    assert not re.search(r"<line [^>]*(class|stroke)", open(plain).read())
    assert '<g id="hatch0">\n<line x1="%s" y1="%s" x2="%s" y2="%s"/>\n' % tuple(svg.fmt(v) for v in h.seg[0]) in open(plain).read()
    stripped = re.sub(r' data-class="[0-3]" stroke="#[0-9a-f]{6}"/>', "/>", text)
    assert stripped == open(plain).read()


@pytest.mark.gpu
def test_render_svg_bolt_with_skin(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "bolt.svg"
    assert ex.main(["bolt", "--layer-height", "8", "--resdiv", "80", "--interpreter", "--hatch", "4", "--skin", "1", "1", "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    sdf = gpu.SDF3HIP(ex.scene("bolt"))
    bb = sdf.Bounds()
    res = ex.spacing(bb, True, 80.0)
    c = ex.trace(gpu, sdf, res, gpu.layer_heights(bb, 8.0))
    sp = np.float32(np.float32(4) * res)
    want = K.skin(S.Loops.of(c), sp, H.directions((45.0, 135.0)), 1, 1)
    assert c.n_layers >= 2 and want.stats["n_segments"] > 0
    assert np.concatenate(svg.read_svg_hatch(str(out))).tobytes() == want.seg.tobytes()
    assert np.concatenate(svg.read_svg_hatch_class(str(out))).tobytes() == want.cls.tobytes()
    assert out.read_text().count("<path ") == c.n_layers
    # the report: every layer's classes, the totals as length x spacing, the overhanging layers, the cost
    assert len(re.findall(r"layer \d+ skin area \(pieces\): inner ", said)) == c.n_layers, said
    m = re.search(r"skin area \(pieces\) in all: inner (\S+) \((\d+)\), bottom (\S+) \((\d+)\), top (\S+) \((\d+)\), both (\S+) \((\d+)\)", said)
    assert m, said
    assert [int(m.group(2 + 2 * q)) for q in range(4)] == want.stats["n_class"]
    for q in range(4):
        assert float(m.group(1 + 2 * q)) == pytest.approx(want.stats["length"][q] * float(sp), rel=1e-8)
    over = [l for l in range(1, c.n_layers) if want.skin_layers[l]["n_segments"][1] or want.skin_layers[l]["n_segments"][3]]
    line = re.search(r"overhangs \(bottom skin above layer 0\): (.*)", said).group(1)
    assert [int(k) for k in re.findall(r"layer (\d+) ", line)] == over and (over or line == "none")
    m = re.search(r"skin: window 1 below, 1 above; (\d+) pieces on (\d+) lines from (\d+) crossings \((\d+) own\), (\d+) of zero length, max_line_crossings (\d+), device time (\S+) ms", said)
    assert m and [int(g) for g in m.groups()[:6]] == [want.stats[f] for f in ("n_segments", "n_lines", "n_crossings", "n_own_crossings", "zero_length", "max_line_crossings")]
    assert float(m.group(7)) > 0


def test_skin_needs_hatch():
    with pytest.raises(SystemExit):
        _example().main(["bolt", "--layer-height", "8", "--skin", "1", "1"])
