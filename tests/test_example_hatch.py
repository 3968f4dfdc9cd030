"""Hatching through examples/render_svg.py and gsdf_amd/svg.py: the file holds one <line> per reported segment, in groups of their
own, and still reads back as the loops of the handle, bit for bit; on the host alone, write_svg(..., hatch=...) followed by read_svg
returns the loops unchanged and read_svg_hatch the segments."""
import importlib.util
import os
import re

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
from gsdf_amd import svg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_write_svg_with_hatching_round_trips_the_loops(tmp_path):
    c = H.hand_loops()
    h = H.hatch(c, 0.5, H.directions((45.0, 135.0)), 0.0437)
    layers = [[l for l, q in zip(c.loops(), c.loop_layer) if q == k] for k in range(c.n_layers)]
    plain, hatched = str(tmp_path / "a.svg"), str(tmp_path / "b.svg")
    svg.write_svg(plain, layers)
    svg.write_svg(hatched, layers, hatch=[h.segments(k) for k in range(c.n_layers)])
    a, b = svg.read_svg(plain), svg.read_svg(hatched)
    assert len(a) == len(b) == c.n_layers
    for la, lb, want in zip(a, b, layers):
        assert len(la) == len(lb) == len(want)
        for x, y, w in zip(la, lb, want):
            assert x.tobytes() == y.tobytes() == np.asarray(w, np.float32).tobytes()
    text = open(hatched).read()
    assert text.count("<line ") == len(h.seg) > 100 and text.count("<path ") == c.n_layers and "<line " not in open(plain).read()
    back = svg.read_svg_hatch(hatched)
    assert len(back) == c.n_layers and np.concatenate(back).tobytes() == h.seg.tobytes()
    assert [len(s) for s in back] == np.diff(h.layer_start.astype(np.int64)).tolist()


@pytest.mark.gpu
def test_render_svg_text_with_hatching(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "text.svg"
    assert ex.main(["text", "--resdiv", "300", "--interpreter", "--hatch", "4", "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    m = re.search(r"hatch: (\d+) segments on (\d+) lines, length (\S+), (\d+) of zero length, max_line_crossings (\d+), device time (\S+) ms", said)
    assert m and "layer 0 hatch:" in said, said
    text = out.read_text()
    assert text.count("<line ") == int(m.group(1)) > 50 and text.count("<path ") == 1
    sdf = gpu.SDF2HIP(ex.scene("text"))
    res = ex.spacing(sdf.Bounds(), False, 300.0)
    c = ex.trace(gpu, sdf, res)
    back = svg.read_svg(str(out))
    assert len(back) == 1 and len(back[0]) == c.n_loops and np.concatenate(back[0]).tobytes() == c.xy.tobytes()
    # the lines of the file are the twin's segments for the traced loops at 45 degrees (one layer: the first angle)
    want = H.hatch(S.Loops.of(c), np.float32(np.float32(4) * res), H.directions((45.0, 135.0)))
    assert np.concatenate(svg.read_svg_hatch(str(out))).tobytes() == want.seg.tobytes()
    assert float(m.group(6)) > 0 and int(m.group(5)) == want.stats["max_line_crossings"]


@pytest.mark.gpu
def test_render_svg_hatches_the_simplified_loops(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "bolt.svg"
    assert ex.main(["bolt", "--layer-height", "8", "--resdiv", "80", "--interpreter", "--simplify", "0.125", "--hatch", "4", "--hatch-angle", "0", "60", "120",
                    "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    sdf = gpu.SDF3HIP(ex.scene("bolt"))
    bb = sdf.Bounds()
    res = ex.spacing(bb, True, 80.0)
    c, _ = ex.trace(gpu, sdf, res, gpu.layer_heights(bb, 8.0)).simplify(np.float32(np.float32(0.125) * res))
    want = H.hatch(S.Loops.of(c), np.float32(np.float32(4) * res), H.directions((0.0, 60.0, 120.0)))
    back = svg.read_svg_hatch(str(out))
    assert len(back) == c.n_layers >= 2 and np.concatenate(back).tobytes() == want.seg.tobytes()
    assert out.read_text().count("<path ") == c.n_layers
    assert len(re.findall(r"layer \d+ hatch: \d+ segments", said)) == c.n_layers and f"hatch: {want.stats['n_segments']} segments" in said
