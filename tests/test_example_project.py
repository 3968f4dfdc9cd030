"""examples/render_ply.py --simplify 4 --project --report as a child process: the projected file has the faces of the mesh without
the projection, byte for byte, and other vertices.

The mesher's record order, and with it the order of the welded faces, differs from one process to the next
(tests/test_gpu_simplify.py::test_example_simplify), so the two files come from ONE process: --before-project writes the mesh as it
was when the projection began. A second run without --project shows that the flag's absence changes nothing: its output is the two
lines it always was, and its file is held to what does not vary between processes (sizes and the faces' edge report)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import toporef as T
import weldref as W
from gsdf_amd import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_render_ply_project(gpu, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "render_ply.py"), "bolt", "--resdiv", "48", "--simplify", "4"]
    before, proj, plain = tmp_path / "before.ply", tmp_path / "projected.ply", tmp_path / "plain.ply"
    r = subprocess.run(cmd + ["--project", "--report", "--before-project", str(before), "-o", str(proj)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v0, i0, n0 = ply.read_ply(before)
    v1, i1, n1 = ply.read_ply(proj)
    assert n0 is None and n1 is None and v0.shape == v1.shape and len(i0) > 0
    assert i1.tobytes() == i0.tobytes()
    assert v1.tobytes() != v0.tobytes()
    assert before.read_bytes()[:len(ply.header(len(v0), len(i0), False))] == proj.read_bytes()[:len(ply.header(len(v1), len(i1), False))]
    assert r.stdout.count(" report: ") == 3 and "bolt projected report: " in r.stdout and "projected onto the field in up to 8 steps: " in r.stdout
    m = re.search(r"bolt deviation: max \|d\| (\S+) -> (\S+) .* from the surface (\d+) -> (\d+) of (\d+)", r.stdout)
    assert m, r.stdout
    assert float(m.group(2)) <= float(m.group(1)) and int(m.group(4)) <= int(m.group(3)) <= int(m.group(5)) == len(v1)
    # the two reports' volumes are those of the two files (printed with nine digits)
    vol = [float(x) for x in re.findall(r"bolt (?:simplified|projected) report: .*?volume (\S+),", r.stdout)]
    want = [T.analyse(v0, i0)["report"]["volume"], T.analyse(v1, i1)["report"]["volume"]]
    print(r.stdout)
    assert len(vol) == 2 and np.allclose(vol, want, rtol=1e-8, atol=0) and vol[0] != vol[1]
    # without --project: the output it always had, and the same mesh up to the mesher's order
    r = subprocess.run(cmd + ["-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "projected" not in r.stdout and "deviation" not in r.stdout and len(r.stdout.strip().splitlines()) == 2
    vp, ip, _ = ply.read_ply(plain)
    assert vp.shape == v0.shape and ip.shape == i0.shape and plain.stat().st_size == before.stat().st_size
    assert W.edge_report(ip) == W.edge_report(i0)
    r = subprocess.run(cmd + ["--before-project", str(plain)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--before-project needs --project" in r.stderr
