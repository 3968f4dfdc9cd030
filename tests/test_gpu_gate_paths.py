"""Whole waves taking each gate's skip, against the oracle (which has no gates), bit for bit.

A D_GATE* (dev_ops.h) skips its child only when all 64 lanes of a wave agree, and the suite's random points never agree: the skip
paths of the evaluator kernels -- R = L, the jump to the child's combine, what the code behind the target finds in the registers and
the LDS columns -- ran for npt-flange's two gates only (tests/test_gpu_wave_votes.py). Here sixteen cases over thirteen small hand-built
trees (tests/gate_paths.py), each pinned to its gate and the combine the gate skips to by an assertion on the lowered program:

    D_GATE2D / D_GATE3D under a union, a difference, a smooth union, a smooth difference; D_GATEZC with the octagon estimate and
    with the cached hypot (D_FLAG_HXY); D_GATEOB behind D_CIRC_ORDER; gates with the context of an enclosing difference, plain and
    smooth; wide unions behind D_UBOUND2D / 3D (the first child's gate against the bound, a later one's against the running
    minimum); a gate behind whose target a position is reloaded and a cylinder recomputes the hypot the gated child replaced.

Points come in clusters, each classified by a float64 restatement of the gate's rule as "every lane passes with ten times the
margin", "no lane passes" or "one lane of a passing wave does not" (first, middle and last lane). The classification is checked
without a GPU (test_every_tree_has_every_class: each class present, nothing unclassified). Every cluster is evaluated
  * by Evaluate on host buffers, 64 points = one wave per call;
  * by evaluate_dev, 1024 points = one tile, whatever the points per lane;
  * by normals against the oracle's central differences (3-D trees);
with the interpreter kernels and with the specialised ones (a per-tree build that fails is a failure), and the interval-stack depth
the handle reports equals the one tests/progcheck.py derives from the program.

Measured on an MI355X: 44 s for the 32 device cases (each specialised case 1-4 s, nearly all of it the per-tree build; each
interpreter case under 0.2 s), 1 s for the 16 classification cases on the CPU. With the wave vote of gate_far changed to "lane 0
decides" (a scratch build) all 32 device cases fail, on their "mixed" clusters.
"""
import numpy as np
import pytest

import gate_paths as G
from oracle.oracle import OracleSDF

F = np.float32
ODD64, ODD1024 = (0, 31, 63), (0, 515, 1023)
CASES = G.cases()
_cache = {}


def _setup(name):
    """(pinned gate, 64-point clusters, 1024-point clusters, oracle) of a case: built once, left unchanged."""
    if name not in _cache:
        case = CASES[name]
        g = G.pin(case)
        _cache[name] = (g, G.clusters(case, g, 64, ODD64), G.clusters(case, g, 1024, ODD1024), OracleSDF(case["shape"].tree()))
    return _cache[name]


def _reference(name):
    """The oracle's distances (and normals) at every cluster's points, computed once per case and shared by the two kernel kinds."""
    key = (name, "ref")
    if key not in _cache:
        g, c64, c1024, ref = _setup(name)
        p64, p1024 = np.concatenate([p for _, _, p in c64]), np.concatenate([p for _, _, p in c1024])
        nrm = ref.normals_central_diff(p64, 1e-3) if CASES[name]["dim"] == 3 else None
        _cache[key] = (p64, ref.Evaluate(p64), p1024, ref.Evaluate(p1024), nrm)
    return _cache[key]


@pytest.mark.parametrize("name", list(CASES))
def test_every_tree_has_every_class(name):
    """No GPU: the gate is the one the case names, and its clusters cover the three classes with none left unclassified."""
    g, c64, c1024, _ = _setup(name)
    for what, cl in (("64", c64), ("1024", c1024)):
        classes = [c for _, c, _ in cl]
        assert None not in classes, (name, what, [l for l, c, _ in cl if c is None])
        assert {"pass", "fail", "mixed"} <= set(classes), (name, what, sorted(set(classes)))
        assert all(p.dtype == F and p.shape[1] == CASES[name]["dim"] for _, _, p in cl)
    # the two sizes agree on what each centre is
    assert [(l, c) for l, c, _ in c64 if "/odd" not in l] == [(l, c) for l, c, _ in c1024 if "/odd" not in l]


def _mismatch(a, b):
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))


def _eval_dev(sdf, pos):
    import torch
    tp = torch.from_numpy(pos).to("cuda").contiguous()
    td = torch.empty(len(pos), device="cuda")
    sdf.evaluate_dev(tp.data_ptr(), pos.shape[1] * 4, td.data_ptr(), len(pos))
    torch.cuda.synchronize()
    return td.cpu().numpy()


def _handle(gpu, name, kind):
    shape = CASES[name]["shape"]
    key = (id(shape), kind)
    if key not in _cache:
        sdf = (gpu.SDF2HIP if CASES[name]["dim"] == 2 else gpu.SDF3HIP)(shape)
        if kind == "specialised":
            sdf.specialize()
        assert sdf.info()["specialized"] == (kind == "specialised"), sdf.info()["kernels"]
        _cache[key] = sdf
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interpreter", "specialised"])
@pytest.mark.parametrize("name", list(CASES))
def test_whole_waves_take_the_skip_like_the_oracle(gpu, name, kind):
    g, c64, c1024, _ = _setup(name)
    p64, want64, p1024, want1024, nrm = _reference(name)
    assert not np.isnan(want64).any() and not np.isnan(want1024).any()    # (so _mismatch masks nothing)
    sdf = _handle(gpu, name, kind)
    # one wave per call
    at = 0
    for label, cls, pts in c64:
        bad = _mismatch(sdf.Evaluate(pts), want64[at:at + len(pts)])
        assert bad.size == 0, (name, kind, "host", label, cls, bad[:8].tolist())
        at += len(pts)
    # one tile per cluster, all tiles in one call
    bad = _mismatch(_eval_dev(sdf, p1024), want1024)
    assert bad.size == 0, (name, kind, "device", [c1024[k][:2] for k in sorted(set((bad // 1024).tolist()))[:4]], bad[:8].tolist())
    if CASES[name]["dim"] == 3:
        bad = _mismatch(sdf.normals(p64, 1e-3).ravel(), nrm.ravel())
        assert bad.size == 0, (name, kind, "normals", [c64[k][:2] for k in sorted(set((bad // 192).tolist()))[:4]])
        assert int(sdf.info()["kernels"]["interval"]) == g["res"].max_lip_depth, (name, sdf.info()["kernels"])
