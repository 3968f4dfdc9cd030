"""examples/render_svg.py end to end: the files it writes read back through gsdf_amd/svg.py as the loops of the handle, bit for
bit -- a 2-D scene's outline and the layers of a 3-D scene -- and the report names every layer."""
import importlib.util
import os
import re

import numpy as np
import pytest

from gsdf_amd import svg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_loops(back, c):
    assert len(back) == c.n_layers
    for k, loops in enumerate(back):
        want = c.loops(k)
        assert len(loops) == len(want), k
        for a, b in zip(loops, want):
            assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all(), k


@pytest.mark.gpu
def test_render_svg_text(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "text.svg"
    assert ex.main(["text", "--resdiv", "300", "--report", "-o", str(out)]) == 0
    said = capsys.readouterr().out
    sdf = gpu.SDF2HIP(ex.scene("text"))
    bb = sdf.Bounds()
    res = ex.spacing(bb, False, 300.0)
    c = ex.trace(gpu, sdf, res)
    assert c.n_loops >= 7  # "Abc123~": seven glyphs, and the counters of A, b, and the others as holes
    _same_loops(svg.read_svg(str(out)), c)
    m = re.search(r"layer 0: (\d+) loops \((\d+) outer, (\d+) holes\), (\d+) vertices", said)
    assert m and (int(m.group(1)), int(m.group(4))) == (c.n_loops, c.n_verts) and int(m.group(3)) >= 2, said
    assert "evaluation" in said and "tracing" in said


@pytest.mark.gpu
def test_render_svg_flange_layers(gpu, tmp_path, capsys):
    ex = _example()
    out = tmp_path / "flange.svg"
    sdf = gpu.SDF3HIP(ex.scene("npt-flange"))
    bb = sdf.Bounds()
    h = float(bb[5] - bb[2]) / 5
    assert ex.main(["npt-flange", "--layer-height", repr(h), "--resdiv", "120", "--interpreter", "-o", str(out)]) == 0
    z = gpu.layer_heights(bb, h)
    res = ex.spacing(bb, True, 120.0)
    c = ex.trace(gpu, sdf, res, z)
    assert c.n_layers == len(z) >= 5 and c.n_loops >= 2 * len(z)
    _same_loops(svg.read_svg(str(out)), c)
    text = out.read_text()
    assert text.count("<path ") == len(z) and text.count('fill-rule="evenodd"') == len(z)
    assert f"{c.n_loops} loops, {c.n_verts} vertices in {len(z)} layer(s)" in capsys.readouterr().out
