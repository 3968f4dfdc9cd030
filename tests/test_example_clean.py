"""examples/render_ply.py --clean: the command line (no device), and the run after --simplify on a device."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from gsdf_amd import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "examples", "render_ply.py")


def load_example():
    spec = importlib.util.spec_from_file_location("render_ply_example", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_arguments():
    ex = load_example()
    a = ex.parse_args(["bolt", "--resdiv", "100", "--simplify", "4", "--clean", "--report"])
    assert (a.scene, a.resdiv, a.simplify, a.clean, a.report, a.project) == ("bolt", 100, 4.0, True, True, None)
    assert ex.parse_args(["bolt"]).clean is False
    assert ex.parse_args(["npt-flange", "--clean", "--adaptive", "0.1", "--project"]).clean is True
    with pytest.raises(SystemExit):
        ex.parse_args(["bolt", "--clean", "yes"])
    with pytest.raises(SystemExit):
        ex.parse_args(["bolt", "--clean", "--before-project", "x.ply"])


@pytest.mark.gpu
def test_example_clean(tmp_path):
    out = tmp_path / "c.ply"
    cmd = [sys.executable, SCRIPT, "bolt", "--resdiv", "100", "--interpreter", "--simplify", "4", "--clean", "--report", "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"^bolt cleaned: V (\d+) -> (\d+), F (\d+) -> (\d+) \((\d+) opposite and (\d+) duplicate faces dropped, (\d+) degenerate; ", r.stdout, re.M)
    assert m, r.stdout
    v_in, v_out, f_in, f_out, opp, dup, deg = map(int, m.groups())
    assert f_out == f_in - opp - dup - deg and opp % 2 == 0 and 0 < f_out <= f_in and 0 < v_out <= v_in
    assert r.stdout.count(" report: ") == 3 and "bolt simplified report: " in r.stdout and "bolt cleaned report: " in r.stdout
    assert r.stdout.index("simplified in cells") < r.stdout.index("bolt cleaned: ") < r.stdout.index("bolt cleaned report: ")
    v, i, n = ply.read_ply(out)
    assert (len(v), len(i)) == (v_out, f_out) and n is None and int(i.max()) == v_out - 1
