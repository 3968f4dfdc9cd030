"""examples/render_ply.py end to end: the file it writes reads back through gsdf_amd/ply.py with the triangle count of the mesher and
the vertex count of the contract's twin."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import weldref as W
from gsdf_amd import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--normals"]])
def test_render_ply_flange_400(gpu, tmp_path, extra):
    out = tmp_path / "f.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "render_ply.py"), "npt-flange", "--resdiv", "400", "-o", str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"V (\d+) F (\d+); PLY (\d+) bytes", r.stdout)
    assert m, r.stdout
    v, idx, nrm = ply.read_ply(out)
    # F from the mesher, V from the twin (tests/test_weld_ref.py: npt-flange at resdiv 400)
    assert (len(v), len(idx)) == (211926, 423852) == (int(m.group(1)), int(m.group(2)))
    # 12 V + 13 F bytes with V = F / 2: 19 per triangle, under half the STL's 50; with normals 25, exactly half plus the header
    assert os.path.getsize(out) == int(m.group(3)) == len(ply.header(len(v), len(idx), bool(extra))) + len(v) * (24 if extra else 12) + 13 * len(idx)
    assert os.path.getsize(out) < (84 + 50 * len(idx)) // 2 + (4096 if extra else 0)
    assert (nrm is not None) == bool(extra) and (nrm is None or np.isfinite(nrm).all())
    assert W.edge_report(idx)["closed_oriented"]
