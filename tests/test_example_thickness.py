"""examples/render_ply.py --thickness: the argument handling and the PLY `quality` property without a device, and one run on the
device -- the example's slab, glyph-plate's base plate (1.0 thick, z = -1.75 .. -0.75, block letters standing on it), through the
example as a child process: the thickness table is printed, the file's `quality` is the twin's thickness over the oracle bit for
bit and is the plate's thickness where the plate is bare, and a file written without --thickness is what it always was."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rayref as R
import weldref as W
from gsdf_amd import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "examples", "render_ply.py")
F = np.float32


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


RESDIV = 100   # res 0.96: a lattice plane falls inside the plate, which is 1.0 thick (at resdiv 48, res 2.0, the bare plate has no vertex)


def plate():
    from scaffold.builder import Builder
    shape = Builder().Scene("glyph-plate")
    res = F(float(shape.Diagonal()) / RESDIV)
    return shape, res, dict(step=res / F(4), t0=res / F(4), tmax=F(shape.Diagonal()), tol=res / F(1024))   # the example's options


def bare_plate(v):
    """(mask, thickness expected) for the vertices on the plate's two faces in the strip between the two rows of letters (y = -3 .. 0;
    half a unit off either row and well inside the plate's rim): the field there is the slab's alone, the inward normal is exactly
    +-z, and the ray from the vertex ends on the other face -- z = -0.75 from below, z = -1.75 from above -- so the thickness is 1.0
    less what the marching-cubes vertex itself is off its face."""
    strip = (v[:, 1] >= -2.5) & (v[:, 1] <= -0.5) & (v[:, 0] >= 0) & (v[:, 0] <= 88)
    below, above = strip & (np.abs(v[:, 2] + 1.75) < 0.25), strip & (np.abs(v[:, 2] + 0.75) < 0.25)
    return below | above, np.where(below, -0.75 - v[:, 2].astype(np.float64), v[:, 2].astype(np.float64) + 1.75)


def bare_least(res):
    """The least number of such vertices: a flat face cuts the lattice's z edges alone, one per lattice column, and a strip 88 x 2
    holds at least floor(88 / res) x floor(2 / res) columns; two faces."""
    return 2 * int(88 / float(res)) * int(2 / float(res))


def test_the_twin_gives_the_bare_plate_its_thickness():
    """Without a device: the twin over the oracle, on the vertices of the oracle's own mesh of the plate. What the device test below
    asks of the example's file is true of the contract."""
    from oracle.oracle import OracleSDF
    shape, res, o = plate()
    cpu = OracleSDF(shape.tree())
    v = np.unique(cpu.render_octree(res).tris.reshape(-1, 3), axis=0)
    bare, want = bare_plate(v)
    th, status, st = R.thickness(cpu.Evaluate, v[bare], **o)
    assert bare.sum() >= bare_least(res) > 300 and (status == R.HIT).all() and (np.abs(th - want[bare]) <= 2 * o["tol"]).all() and (np.abs(th - 1) < 0.25).all()


def test_arguments_without_a_device():
    """Refused on the command line, before any device is touched."""
    for argv, word in ((["bolt", "--thickness", "-1"], "--thickness needs a THIN >= 0"), (["bolt", "--thickness", "nan"], "--thickness needs a THIN >= 0"),
                       (["bolt", "--thickness", "thin"], "invalid float value")):
        r = subprocess.run([sys.executable, EXAMPLE] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr)
    r = subprocess.run([sys.executable, EXAMPLE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--thickness [THIN]" in r.stdout and "quality" in r.stdout


def test_quality_round_trips_and_files_without_it_are_unchanged():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    i = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)
    n = np.array([[-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    q = np.array([0.25, np.inf, 0, -0.0], F)
    q[2] = np.array([0x7fc00000], np.uint32).view(F)[0]
    for nrm in (None, n):
        plain = ply.ply_bytes(v, i, nrm)
        assert plain == ply.header(4, 4, nrm is not None) + (v if nrm is None else np.concatenate([v, n], axis=1)).tobytes() + plain[-52:]
        assert b"quality" not in plain and ply.ply_bytes(v, i, nrm, quality=None) == plain
        withq = ply.ply_bytes(v, i, nrm, quality=q)
        names = re.findall(rb"property float (\w+)", withq)
        assert names == [b"x", b"y", b"z"] + ([b"nx", b"ny", b"nz"] if nrm is not None else []) + [b"quality"]   # behind the normals
        assert len(withq) - len(plain) == len(ply.header(4, 4, nrm is not None, True)) - len(ply.header(4, 4, nrm is not None)) + 16
        v2, i2, n2, q2 = ply.parse_ply(withq, quality=True)
        assert (u32(v2) == u32(v)).all() and (i2 == i).all() and (u32(q2) == u32(q)).all() and ((n2 is None) if nrm is None else (u32(n2) == u32(n)).all())
        assert len(ply.parse_ply(withq)) == 3 and (u32(ply.parse_ply(withq)[0]) == u32(v)).all()    # the three values it always returned
        assert ply.parse_ply(plain, quality=True)[3] is None and len(ply.parse_ply(plain)) == 3
    with pytest.raises(ValueError):
        ply.ply_bytes(v, i, quality=q[:3])


@pytest.mark.gpu
def test_render_ply_thickness(gpu, tmp_path):
    from oracle.oracle import OracleSDF
    cmd = [sys.executable, EXAMPLE, "glyph-plate", "--resdiv", str(RESDIV), "--interpreter"]
    thick, plain = tmp_path / "thick.ply", tmp_path / "plain.ply"
    r = subprocess.run(cmd + ["--thickness", "0.5", "--report", "-o", str(thick)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"glyph-plate thickness: min (\S+), max (\S+) \(.*\); (\d+) of (\d+) vertices below 0.5; (.*?); (\d+) evaluations", r.stdout)
    assert m, r.stdout
    v, i, n, q = ply.read_ply(thick, quality=True)
    assert n is None and q is not None and len(q) == len(v) == int(m.group(4)) and len(i) > 0
    # the values: the twin's over the oracle for the file's vertices, bit for bit (the status table and the evaluations too) ...
    shape, res, o = plate()
    counted = R.CountingSDF(OracleSDF(shape.tree()).Evaluate)
    th, status, st = R.thickness(counted, v, thin=0.5, **o)
    assert (u32(q) == u32(th)).all(), np.flatnonzero(u32(q) != u32(th))[:8].tolist()
    table = dict((w.rsplit(" ", 1)[0], int(w.rsplit(" ", 1)[1])) for w in m.group(5).split(", "))
    assert table == {R.STATUS[k].lower(): int(c) for k, c in enumerate(st["count"]) if c} and int(m.group(6)) == st["evals"] == counted.count
    assert int(m.group(3)) == st["below"] and float(m.group(1)) == pytest.approx(float(st["t_min"]), rel=1e-5) and float(m.group(2)) == pytest.approx(float(st["t_max"]), rel=1e-5)
    # ... and where the plate is bare, the plate's thickness
    bare, want = bare_plate(v)
    assert bare.sum() >= bare_least(res) and (np.abs(q[bare] - want[bare]) <= 2 * o["tol"]).all() and (np.abs(q[bare] - 1) < 0.25).all()
    # the device again on the file's vertices: the same bytes
    ix = gpu.IndexedHIP.from_arrays(v, i)
    th2, _, st2 = ix.thickness(gpu.SDF3HIP(shape), thin=F(0.5), **o)
    assert (u32(th2) == u32(q)).all() and st2.result_bytes() == R.stats_bytes(st)
    # without --thickness: the output and the file it always had (the library's own bytes: ply_bytes without quality)
    r = subprocess.run(cmd + ["-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " thickness: " not in r.stdout and len(r.stdout.strip().splitlines()) == 1   # (the file's path may hold the word)
    vp, ip, np_ = ply.read_ply(plain)
    assert plain.read_bytes() == ply.ply_bytes(vp, ip) and b"quality" not in plain.read_bytes()
    assert vp.shape == v.shape and ip.shape == i.shape and W.edge_report(ip) == W.edge_report(i)
    assert thick.read_bytes() == ply.ply_bytes(v, i, quality=q)
