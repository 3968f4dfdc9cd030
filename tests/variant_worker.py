"""One process under a forced kernel variant (tests/test_gpu_variants.py starts it with GSDF_HIP_BATCH_K, GSDF_HIP_SWEEP_WAVES or
GSDF_HIP_LEAF_WAVES set: each is read once per process): the five example scenes -- brick masks, the sector gate, the polygon
culling -- through Evaluate on both host-buffer paths, the octree, the flat renderer and dual contouring, against the oracle bit
for bit. Prints the kernel names of every handle ("kernels <scene> <names>") and "variants ok" at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from gsdf_amd import hip  # noqa: E402
from oracle.oracle import OracleSDF  # noqa: E402
from scaffold.builder import Builder  # noqa: E402

SCENES = ["npt-flange", "bolt", "knurled-cylinder", "glyph-plate", "fibonacci-showerhead"]
SMALL_CALL = 262144   # host-buffer calls up to here run eval_kernel<D,1,4> whatever the handle's K (abi_eval.hip: eval_submit)


def sorted_bits(t):
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])].view(np.uint32)


def same(got, want, what):
    got, want = sorted_bits(got), sorted_bits(want)
    assert got.shape == want.shape and (got == want).all(), (what, got.shape, want.shape)


def main():
    assert any(os.environ.get(k) for k in ("GSDF_HIP_BATCH_K", "GSDF_HIP_SWEEP_WAVES", "GSDF_HIP_LEAF_WAVES"))
    hip.init(0)
    b = Builder()
    rng = np.random.default_rng(3)
    for name in SCENES:
        s = b.Scene(name)
        cpu, sdf = OracleSDF(s.tree()), hip.SDF3HIP(s)
        bb = s.Bounds().astype(np.float32)
        c, h = (bb[:3] + bb[3:]) / 2, (bb[3:] - bb[:3]) / 2 * np.float32(1.1)
        pos = (c + (rng.random((SMALL_CALL + 257, 3), np.float32) * 2 - 1) * h).astype(np.float32)   # ragged for K = 4, 2 and 1
        want = cpu.Evaluate(pos)
        for n in (2049, len(pos)):      # the one-point-per-lane kernel of small calls; the handle's own above the threshold
            got = sdf.Evaluate(pos[:n].copy())
            bad = int(((got.view(np.uint32) != want[:n].view(np.uint32)) & ~(np.isnan(got) & np.isnan(want[:n]))).sum())
            assert bad == 0, (name, n, bad)
        res = np.float32(float(s.Diagonal()) / 60)
        m = cpu.render_octree(res, 4096, True)
        for kw in ({}, {"prune": False}, {"share_corners": 1}, {"share_corners": 2}):
            oc = hip.OctreeHIP(sdf, res, **kw)
            assert oc.n_tris() == m.n_tris, (name, kw, oc.n_tris(), m.n_tris)
            same(oc.RenderAll(), m.tris, (name, "octree", kw))
        fl, mf = hip.FlatHIP(sdf, res), cpu.render_flat(res, 4096, 2)
        assert fl.Evaluations() == mf.evals and fl.n_tris() == mf.n_tris, (name, "flat", fl.Evaluations(), mf.evals)
        same(fl.RenderAll(), mf.tris, (name, "flat"))
        md = cpu.render_dualcontour(res, False)
        same(hip.DualContourHIP(sdf, res).RenderAll(), md.tris, (name, "dual contouring"))
        print("kernels", name, " ".join(f"{k}={v}" for k, v in sdf.info()["kernels"].items() if k != "code"), m.n_tris, mf.n_tris, md.n_tris, flush=True)
    print("variants ok")


if __name__ == "__main__":
    main()
