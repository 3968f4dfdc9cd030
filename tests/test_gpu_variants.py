"""Every interpreter kernel variant against the oracle, op by op.

A handle picks its kernels' template arguments from the tree's LDS slot count (abi_program.h: batch_k, sweep_waves, leaf_config), and
the suite's own trees stay in the class of the smallest (tests/test_variant_census.py has the table). Here every corpus shape is
lifted (tests/slot_ladder.py) into every slot class, the oracle evaluates the same lifted tree, and every comparison is bit for bit
(the bezier shape: test_gpu_eval.py's REL_TOL). Each case asserts, from a literal table, which kernels gsdf_hip_program_kernels names
for its rung. Between them the assertions name every instantiation:

  eval_kernel<3,4,4> <3,4,3> <3,2,4> <3,2,3> <3,1,4>, eval_kernel<2,4,4> <2,4,3> <2,2,4> <2,2,3> <2,1,4>           (a; <D,1,4> is also
                                                                              what every host-buffer call of (a) runs, on every tree)
  leaf_eval_kernel<4,3> (rungs 9-11 of a) <2,3> <1,4>, prune_kernel, flat_grid_kernel<4,3> <2,4> <2,3> <1,4>,
  dc_origin_kernel<4,3> <2,3> <1,4>, project_kernel                                                                 (b)
  image2_kernel<4> <2> <1>, image2_color_kernel<4,kind> <2,kind> <1,kind>                                           (b, 2-D)
  eval_kernel<3,2,4> <3,1,4> <3,4,3>, leaf_eval_kernel<2,3> <1,4> <4,2> on the example scenes                        (c, forced)
  the specialised builds of eval / leaf / prune for one lifted tree per class                                       (d)

Time, one run on one MI355X machine: this file 40 s (38 cases), straight after it the rest of the GPU suite (338 cases, which is the
parent commit's suite) 596 s. Per case: every op of a dimension in one class 0.15-0.4 s (40 to 45 trees, four evaluations each), the
meshers per rung 0.3-0.7 s (six trees, all entry points), image and picture per rung 0.02-0.03 s, the limit cases below 1 s, a
forced-variant child process 2.9-3.2 s, the specialised builds 1.9 / 2.2 / 2.8 / 6.7 s, the slowest.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
import dcref
import slot_ladder as SL
import viewref
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_eval import REL_TOL
from test_gpu_picture import _check_picture
from test_gpu_project import check as check_project, opts_for
from test_gpu_view import _same as same_frame

pytestmark = pytest.mark.gpu
F = np.float32

# rung -> (K, W) of the eval sweep; the leaf phase's evaluating kernel; the flat renderer's lattice pass; dual contouring's origin sweep.
# Literal on purpose: the test states which kernel a rung is meant to reach, the library reports which one it launches.
EVAL_KW = {9: (4, 4), 10: (4, 3), 11: (4, 3), 12: (4, 3), 13: (2, 4), 19: (2, 4), 20: (2, 3), 21: (2, 3), 28: (2, 3), 29: (1, 4), 40: (1, 4)}
LEAF = {9: "leaf_eval_kernel<4,3>", 10: "leaf_eval_kernel<4,3>", 11: "leaf_eval_kernel<4,3>", 12: "leaf_eval_kernel<2,3>", 13: "leaf_eval_kernel<2,3>",
        19: "leaf_eval_kernel<2,3>", 20: "leaf_eval_kernel<2,3>", 21: "leaf_eval_kernel<2,3>", 28: "leaf_eval_kernel<2,3>", 29: "leaf_eval_kernel<1,4>",
        40: "leaf_eval_kernel<1,4>"}
FLAT = {12: "flat_grid_kernel<4,3>", 13: "flat_grid_kernel<2,4>", 19: "flat_grid_kernel<2,4>", 20: "flat_grid_kernel<2,3>", 21: "flat_grid_kernel<2,3>",
        28: "flat_grid_kernel<2,3>", 29: "flat_grid_kernel<1,4>", 40: "flat_grid_kernel<1,4>"}
DC = {12: "dc_origin_kernel<4,3>", 13: "dc_origin_kernel<2,3>", 19: "dc_origin_kernel<2,3>", 20: "dc_origin_kernel<2,3>", 21: "dc_origin_kernel<2,3>",
      28: "dc_origin_kernel<2,3>", 29: "dc_origin_kernel<1,4>", 40: "dc_origin_kernel<1,4>"}
IMAGE_K = {12: 4, 13: 2, 19: 2, 20: 2, 21: 2, 28: 2, 29: 1, 40: 1}
N = 2049   # two tiles of 1024 points (K = 4) and one point: ragged for K = 4, 2 and 1


def _mismatch(a, b):
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def _mismatch_ref(dev, ref):
    """_mismatch, with the relation of tests/test_gpu_nan.py where the REFERENCE is NaN: its minima and maxima hand a NaN on
    (math32.Min / Max), the device's drop it (v_min_f32 / v_max_f32), so under a chain of Xor / Difference links a NaN of the
    innermost shape stays NaN in the oracle and becomes a stand-in on the device. Bit for bit wherever the reference is a number;
    _check_eval asserts how many points that leaves out: none, but two of the 2049 for the ellipse (l = 0 on an axis: 0 / 0)."""
    return int(((dev.view(np.uint32) != ref.view(np.uint32)) & ~np.isnan(ref)).sum())


def _sorted(t):
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])].view(np.uint32)


def _same_tris(got, want, what):
    """Bit for bit as sorted triangles; a failure names how many differ and shows three of them as floats."""
    got, want = _sorted(got), _sorted(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), got[bad[:3]].view(np.float32), want[bad[:3]].view(np.float32))


def _points(base, seed):
    """N points over the BASE shape's bounds (corpus.sample_points: lattice with the exact zeros and edges, uniform points 25 % past
    the bounds, the axis points) plus points of the 0.125 lattice, as the fuzz test adds."""
    dim = 2 if base.is2d else 3
    p = corpus.sample_points(base, n_grid=7 if dim == 3 else 9, n_rand=1500)
    g = F(0.125) * np.random.default_rng(seed).integers(-12, 13, (N - len(p), dim)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([p, g]).astype(np.float32))


def _check_eval(gpu, sdf, pos, want, what, stride16, tol=False, nan_points=0):
    """Host-buffer Evaluate of N points (eval_kernel<D,1,4>, ragged last tile) and evaluate_dev on device tensors at 1, 1024 and N
    points (the handle's own kernel: one lane, one exact tile of K = 4, ragged tiles), 16-byte stride too where asked. nan_points:
    at how many points the reference is NaN (_mismatch_ref leaves exactly those out): none, unless the caller says so."""
    import torch
    assert int(np.isnan(want).sum()) == nan_points, (what, int(np.isnan(want).sum()), nan_points)

    def same(got, n, how):
        if tol:
            assert np.max(np.abs(got - want[:n]) / np.maximum(np.abs(want[:n]), 1e-3)) <= REL_TOL, (what, how, n)
        else:
            assert _mismatch_ref(got, want[:n]) == 0, (what, how, n, _mismatch_ref(got, want[:n]))
    same(sdf.Evaluate(pos), N, "host buffer")
    dim = pos.shape[1]
    layouts = [(pos, 4 * dim)]
    if stride16:
        wide = np.full((N, 4), 123.0, np.float32)
        wide[:, :dim] = pos
        layouts.append((wide, 16))
    for arr, stride in layouts:
        tp = torch.from_numpy(arr).cuda()
        for n in (1, 1024, N):
            td = torch.full((N,), float("nan"), device="cuda")
            torch.cuda.synchronize()
            sdf.evaluate_dev(tp.data_ptr(), stride, td.data_ptr(), n)      # (enqueued on the handle's own stream: wait for it)
            torch.cuda.synchronize()
            out = td.cpu().numpy()
            same(out[:n], n, ("device", stride))
            assert np.isnan(out[n:]).all(), (what, "wrote past n", n, stride)


# ---- (a) every op under every eval instantiation

@pytest.mark.parametrize("cls", range(len(SL.CLASSES)), ids=[c[0] for c in SL.CLASSES])
@pytest.mark.parametrize("dim", [3, 2])
def test_every_op_under_every_eval_variant(gpu, dim, cls):
    b = Builder()
    bases = dict(corpus.shapes3d(b)[1] if dim == 3 else corpus.shapes2d(b)[1] + corpus.bezier2d(b)[1])
    rungs = set()
    for k, (name, rung, sh) in enumerate(SL.eval_cases(b, dim, cls)):
        sdf = gpu.SDFHIP(sh)
        info = sdf.info()
        assert info["lds_slots"] == rung, (name, rung, info["lds_slots"])
        assert info["kernels"]["eval"] == "eval_kernel<%d,%d,%d>:interpreter" % ((dim,) + EVAL_KW[rung]), (name, rung, info["kernels"])
        if dim == 3:
            assert info["kernels"]["leaf"] == LEAF[rung] + ":interpreter", (name, rung, info["kernels"])
        pos = _points(bases[name], k)
        want = OracleSDF(sh.tree()).Evaluate(pos)
        _check_eval(gpu, sdf, pos, want, (name, rung), stride16=rung not in rungs, tol=name == "quadbezier", nan_points=2 if name == "ellipse" else 0)
        rungs.add(rung)
    assert rungs == set(SL.CLASS_RUNGS[cls])


# ---- (b) the other kernels that carry a K

def _mesh_checks(gpu, name, sh, sdf, what):
    cpu = OracleSDF(sh.tree())
    res = F(float(sh.Diagonal()) / 32)
    m = cpu.render_octree(res, 4096, True)
    assert m.n_tris > 0, what
    # (share_corners 1 and 2 have kernels of their own at four points per lane only, that is up to 11 slots: from rung 12 on they must
    # come out as the default does; the dense and rows kernels themselves run in the forced-variant children of part (c))
    for kw in ({}, {"prune": False}, {"share_corners": 1}, {"share_corners": 2}):
        oc = gpu.OctreeHIP(sdf, res, **kw)
        assert oc.n_tris() == m.n_tris, (what, kw, oc.n_tris(), m.n_tris)
        _same_tris(oc.RenderAll(), m.tris, (what, "octree", kw))
        if not kw:
            assert oc.TotalPruned() == m.pruned, (what, oc.TotalPruned(), m.pruned)
    rec = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
    assert rec.payload()[0] == gpu.PAYLOAD_RECORDS
    ix = rec.weld()                                          # (the welded mesh of the records: what project() moves below)
    rec.march()
    _same_tris(rec.RenderAll(), m.tris, (what, "records marched"))
    fl, mf = gpu.FlatHIP(sdf, res), cpu.render_flat(res, 4096, 2)
    assert fl.Evaluations() == mf.evals and fl.n_tris() == mf.n_tris, (what, "flat", fl.Evaluations(), mf.evals, fl.n_tris(), mf.n_tris)
    _same_tris(fl.RenderAll(), mf.tris, (what, "flat"))
    # dual contouring: the soup against the oracle's, the indexed mesh against the twin over the oracle (dcref.py)
    tv, ti, tk, _, _, ref = dcref.mesh(cpu, res, False)
    _same_tris(gpu.DualContourHIP(sdf, res).RenderAll(), ref.tris, (what, "dual contouring"))
    dx = gpu.IndexedHIP.dual_contour(sdf, res)
    v, i, k = dx.read()
    assert (k.tobytes(), i.tobytes(), v.tobytes()) == (tk.tobytes(), ti.tobytes(), tv.tobytes()), (what, "dual contouring, indexed", dx.n_verts, len(tv), dx.n_tris, len(ti))
    pos = corpus.sample_points(sh, n_grid=4, n_rand=500)
    assert _mismatch(sdf.normals(pos, 1e-3).ravel(), cpu.normals_central_diff(pos, 1e-3).ravel()) == 0, (what, "normals")
    view = gpu.view_orbit(sh.Bounds(), 0.6, 0.35)
    same_frame(sdf.render3(view, 32, 24), viewref.render(cpu.Evaluate, view, 32, 24), (what, "render3"))
    verts = ix.read()[0]
    for iters in (0, 2):
        check_project(ix, sdf, cpu.Evaluate, verts, (what, "project"), **opts_for(res, iters))
    return m.n_tris


@pytest.mark.parametrize("rung", SL.MESH_RUNGS)
def test_meshers_normals_view_and_projection_per_rung(gpu, rung):
    b = Builder()
    for name, base in SL.mesh_bases(b):
        sh = SL.lift(b, base, rung)
        sdf = gpu.SDF3HIP(sh)
        kern = sdf.info()["kernels"]
        assert sdf.info()["lds_slots"] == rung
        want = {"eval": "eval_kernel<3,%d,%d>:interpreter" % EVAL_KW[rung], "leaf": LEAF[rung] + ":interpreter", "prune": "prune_kernel:interpreter",
                "flat": FLAT[rung] + ":interpreter", "dc": DC[rung] + ":interpreter", "project": "project_kernel:interpreter"}
        assert {k: kern[k] for k in want} == want, (name, rung, kern)
        _mesh_checks(gpu, name, sh, sdf, (name, rung))


@pytest.mark.parametrize("rung", SL.MESH_RUNGS)
def test_image_and_picture_per_rung(gpu, rung):
    b = Builder()
    for name, base in SL.image_bases(b):
        sh = SL.lift(b, base, rung)
        sdf = gpu.SDF2HIP(sh)
        kern = sdf.info()["kernels"]
        want = {"eval": "eval_kernel<2,%d,%d>:interpreter" % EVAL_KW[rung], "image": "image2_kernel<%d>:interpreter" % IMAGE_K[rung],
                "picture": "image2_color_kernel<%d,kind>:interpreter" % IMAGE_K[rung]}
        assert {k: kern[k] for k in want} == want, (name, rung, kern)
        dg, cg = sdf.render_image(48, 32)
        dc_, cc = OracleSDF(sh.tree()).render_image(48, 32)
        assert _mismatch(dg.ravel(), dc_.ravel()) == 0 and (cg == cc).all(), (name, rung, "render_image")
        _check_picture(gpu, sdf, sh.tree(), 48, 32, (name, rung))


# ---- (c) real trees under forced variants

# what the knob forces on the example scenes (all of them <= 10 slots: K = 4 by default). GSDF_HIP_LEAF_WAVES: leaf_config honours 2, 4
# and 5 at K = 4; 2 alone selects another ahead-of-time kernel (<4,2> for <4,3>), 4 and 5 are occupancies of specialised builds and must
# leave the interpreter on <4,3>. At K = 2 it honours 4, likewise for specialised builds only (the interpreter has <2,3> alone, run
# under GSDF_HIP_BATCH_K=2); that pair of knobs would be a seventh child and is not run.
FORCED = {"GSDF_HIP_BATCH_K=2": ("eval_kernel<3,2,4>", "leaf_eval_kernel<2,3>", "flat_grid_kernel<2,4>", "dc_origin_kernel<2,3>"),
          "GSDF_HIP_BATCH_K=1": ("eval_kernel<3,1,4>", "leaf_eval_kernel<1,4>", "flat_grid_kernel<1,4>", "dc_origin_kernel<1,4>"),
          "GSDF_HIP_SWEEP_WAVES=3": ("eval_kernel<3,4,3>", "leaf_eval_kernel<4,3>", "flat_grid_kernel<4,3>", "dc_origin_kernel<4,3>"),
          "GSDF_HIP_LEAF_WAVES=2": ("eval_kernel<3,4,4>", "leaf_eval_kernel<4,2>", "flat_grid_kernel<4,4>", "dc_origin_kernel<4,3>"),
          "GSDF_HIP_LEAF_WAVES=4": ("eval_kernel<3,4,4>", "leaf_eval_kernel<4,3>", "flat_grid_kernel<4,4>", "dc_origin_kernel<4,3>"),
          "GSDF_HIP_LEAF_WAVES=5": ("eval_kernel<3,4,4>", "leaf_eval_kernel<4,3>", "flat_grid_kernel<4,4>", "dc_origin_kernel<4,3>")}
TEN_SLOTS = {"knurled-cylinder": ("eval_kernel<3,4,3>", "flat_grid_kernel<4,3>")}   # its sweeps run three workgroups per CU unless K is forced down


@pytest.mark.parametrize("knob", sorted(FORCED))
def test_example_scenes_under_a_forced_variant(gpu, knob):
    """The knobs are statics read once per process: tests/variant_worker.py is that process, one at a time."""
    key, val = knob.split("=")
    env = {k: v for k, v in os.environ.items() if k not in ("GSDF_HIP_BATCH_K", "GSDF_HIP_SWEEP_WAVES", "GSDF_HIP_LEAF_WAVES")}
    env[key] = val
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "variant_worker.py")
    pr = subprocess.run([sys.executable, worker], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = pr.stdout.decode(errors="replace")
    print(out[-3000:])
    assert pr.returncode == 0 and "variants ok" in out, out[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("kernels ")]
    assert len(lines) == 5
    e, lf, fg, dc = FORCED[knob]
    for ln in lines:
        kern = dict(kv.split("=") for kv in ln.split()[2:] if "=" in kv)
        e1, fg1 = TEN_SLOTS.get(ln.split()[1], (e, fg)) if key == "GSDF_HIP_LEAF_WAVES" else (e, fg)
        assert (kern["eval"], kern["leaf"], kern["flat"], kern["dc"]) == tuple(x + ":interpreter" for x in (e1, lf, fg1, dc)), ln


# ---- (d) specialised kernels

SPECIALISED = [("torus", 12), ("box", 20), ("cyl0", 28), ("sphere", 40)]


@pytest.mark.parametrize("name,rung", SPECIALISED)
def test_specialised_build_of_a_lifted_tree(gpu, name, rung):
    """specialize() of one lifted tree per class above the first: the checks of (a) and an octree mesh through the tree's own kernels.
    Measured: specialize() 1.2 s (torus, 12 slots), 1.5 s (box, 20), 1.9 s (cylinder, 28), 6.5 s (sphere, 40); the cases 1.9 / 2.2 / 2.8 / 6.7 s."""
    b = Builder()
    base = dict(corpus.shapes3d(b)[1])[name]
    sh = SL.lift(b, base, rung)
    sdf = gpu.SDF3HIP(sh).specialize()
    info = sdf.info()
    print(name, rung, "specialize() took %.1f s" % info["specialize_s"], info["kernels"])
    k = EVAL_KW[rung][0]
    assert info["specialized"] and info["kernels"]["eval"].startswith("eval_kernel<3,%d," % k) and info["kernels"]["eval"].endswith(":specialised"), info["kernels"]
    assert info["kernels"]["leaf"].endswith(":specialised") and info["kernels"]["prune"] == "prune_kernel:specialised", info["kernels"]
    cpu = OracleSDF(sh.tree())
    pos = _points(base, rung)
    _check_eval(gpu, sdf, pos, cpu.Evaluate(pos), (name, rung, "specialised"), stride16=True)
    res = F(float(sh.Diagonal()) / 32)
    m = cpu.render_octree(res, 4096, True)
    oc = gpu.OctreeHIP(sdf, res)
    assert oc.n_tris() == m.n_tris > 0
    _same_tris(oc.RenderAll(), m.tris, (name, rung, "octree, specialised"))


# ---- (e) the largest trees (include/gsdf_hip.h: "Largest trees")

BAD_TREE = -4


def _refused(gpu, call, limit):
    with pytest.raises(gpu.HipError) as e:
        call()
    assert e.value.code == BAD_TREE and limit in e.value.msg and "LDS" in e.value.msg, (e.value.code, e.value.msg)


def _still_usable(gpu, b):
    s = b.NewSphere(1)
    pos = corpus.sample_points(s, n_grid=4, n_rand=200)
    assert _mismatch(gpu.SDF3HIP(s).Evaluate(pos), OracleSDF(s.tree()).Evaluate(pos)) == 0


def test_largest_tree_every_entry_point_takes(gpu):
    """51 slots under an interval stack of 16: what every entry point accepts (the octree counts both: 67), with the oracle's bits
    from each of them. 2-D trees have no limit but creation's."""
    b = Builder()
    base = dict(corpus.shapes3d(b)[1])["torus"]
    sh = SL.lift(b, base, 51)
    sdf = gpu.SDF3HIP(sh)
    assert sdf.info()["lds_slots"] == 51 and int(sdf.info()["kernels"]["interval"]) == 16      # (sixteen brick-mask frames nest in the chain)
    pos = _points(base, 51)
    _check_eval(gpu, sdf, pos, OracleSDF(sh.tree()).Evaluate(pos), ("torus", 51), stride16=True)
    _mesh_checks(gpu, "torus", sh, sdf, ("torus", 51))


def test_one_slot_more_is_refused_on_the_host_and_the_library_stays_usable(gpu):
    """Each limit from both sides: the tree at the limit gives the oracle's bits, the tree one slot above is refused with
    GSDF_ERR_BAD_TREE and a message that names the limit -- by a check on the host: no launch asks for more LDS than a CU has -- and
    the handle (its other entry points) and the library (the next small tree) work on."""
    b = Builder()
    base = b.NewSphere(1)
    pos = _points(base, 1)
    small = corpus.sample_points(base, n_grid=4, n_rand=300)

    def handle(n):
        sh = SL.lift(b, base, n)
        sdf = gpu.SDF3HIP(sh)
        assert sdf.info()["lds_slots"] == n
        return sh, sdf, OracleSDF(sh.tree())

    # the octree: slots + interval stack <= 67 (at 67: the test above); dual contouring: 52 slots
    sh, sdf, cpu = handle(52)
    assert 52 + int(sdf.info()["kernels"]["interval"]) == 68
    res = F(float(sh.Diagonal()) / 32)
    _same_tris(gpu.DualContourHIP(sdf, res).RenderAll(), cpu.render_dualcontour(res, False).tris, "dual contouring at 52 slots")
    _refused(gpu, lambda: gpu.OctreeHIP(sdf, res), "<= 67")
    _refused(gpu, lambda: gpu.OctreeHIP(sdf, res, prune=False, payload=gpu.PAYLOAD_RECORDS), "<= 67")
    assert _mismatch(sdf.normals(small, 1e-3).ravel(), cpu.normals_central_diff(small, 1e-3).ravel()) == 0
    _still_usable(gpu, b)
    sh, sdf, cpu = handle(53)
    res = F(float(sh.Diagonal()) / 32)
    _refused(gpu, lambda: gpu.DualContourHIP(sdf, res), "52 slots")
    _refused(gpu, lambda: gpu.IndexedHIP.dual_contour(sdf, res), "52 slots")
    assert _mismatch(sdf.Evaluate(pos), cpu.Evaluate(pos)) == 0
    _still_usable(gpu, b)
    # normals and projection: 80 slots
    sh, sdf, cpu = handle(80)
    assert _mismatch(sdf.normals(small, 1e-3).ravel(), cpu.normals_central_diff(small, 1e-3).ravel()) == 0
    v, i = np.ascontiguousarray(small[:300]), np.arange(300, dtype=np.uint32).reshape(-1, 3)
    ix = gpu.IndexedHIP.from_arrays(v, i)
    o = dict(step=F(0.01), tol=F(1e-4), max_move=F(0.5))
    for iters in (0, 2):
        check_project(ix, sdf, cpu.Evaluate, v, "project at 80 slots", max_iters=iters, **o)
    sh, sdf, cpu = handle(81)
    _refused(gpu, lambda: sdf.normals(small, 1e-3), "80 slots")
    _refused(gpu, lambda: ix.project(sdf, max_iters=2, **o), "80 slots")
    _refused(gpu, lambda: ix.normals(sdf, 1e-3), "80 slots")
    view = gpu.view_orbit(sh.Bounds(), 0.6, 0.35)
    same_frame(sdf.render3(view, 32, 24), viewref.render(cpu.Evaluate, view, 32, 24), "render3 at 81 slots")
    fres = F(float(sh.Diagonal()) / 24)
    fl, mf = gpu.FlatHIP(sdf, fres), cpu.render_flat(fres, 4096, 2)
    assert fl.Evaluations() == mf.evals
    _same_tris(fl.RenderAll(), mf.tris, "flat at 81 slots")
    _still_usable(gpu, b)
    # creation: 143 slots, and what a handle that exists does whatever its size: evaluate, render3, the flat renderer (3-D) ...
    sh, sdf, cpu = handle(143)
    _check_eval(gpu, sdf, pos, cpu.Evaluate(pos), "143 slots", stride16=False)
    view = gpu.view_orbit(sh.Bounds(), 0.6, 0.35)
    same_frame(sdf.render3(view, 32, 24), viewref.render(cpu.Evaluate, view, 32, 24), "render3 at 143 slots")
    fres = F(float(sh.Diagonal()) / 24)
    fl, mf = gpu.FlatHIP(sdf, fres), cpu.render_flat(fres, 4096, 2)
    assert fl.Evaluations() == mf.evals and mf.n_tris > 0
    _same_tris(fl.RenderAll(), mf.tris, "flat at 143 slots")
    with pytest.raises(gpu.HipError) as e:
        gpu.SDF3HIP(SL.lift(b, base, 144))
    assert e.value.code == BAD_TREE, (e.value.code, e.value.msg)
    _still_usable(gpu, b)
    # ... evaluate, the image and the picture (2-D)
    base2 = b.NewCircle(1)
    sh2 = SL.lift(b, base2, 143)
    sdf2 = gpu.SDF2HIP(sh2)
    kern = sdf2.info()["kernels"]
    assert sdf2.info()["lds_slots"] == 143 and (kern["eval"], kern["image"], kern["picture"]) == \
        ("eval_kernel<2,1,4>:interpreter", "image2_kernel<1>:interpreter", "image2_color_kernel<1,kind>:interpreter"), kern
    pos2 = _points(base2, 2)
    _check_eval(gpu, sdf2, pos2, OracleSDF(sh2.tree()).Evaluate(pos2), "143 slots, 2-D", stride16=False)
    dg, cg = sdf2.render_image(48, 32)
    dc_, cc = OracleSDF(sh2.tree()).render_image(48, 32)
    assert _mismatch(dg.ravel(), dc_.ravel()) == 0 and (cg == cc).all(), "render_image at 143 slots"
    _check_picture(gpu, sdf2, sh2.tree(), 48, 32, "picture at 143 slots")
    with pytest.raises(gpu.HipError) as e:
        gpu.SDF2HIP(SL.lift(b, base2, 144))
    assert e.value.code == BAD_TREE, (e.value.code, e.value.msg)
    pos2s = corpus.sample_points(base2, n_grid=5, n_rand=100)
    assert _mismatch(gpu.SDF2HIP(base2).Evaluate(pos2s), OracleSDF(base2.tree()).Evaluate(pos2s)) == 0
