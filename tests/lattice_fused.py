"""One process under GSDF_HIP_FUSED_LEAF=1 (tests/test_gpu_lattice.py starts it): the fused leaf kernels -- leaf_kernel with
mc_emit_balanced, and leaf_brick_kernel with mc_emit_block under share_corners = 1 -- on lattice-aligned members, against the
oracle bit for bit. Prints "fused ok" at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import lattice_trees as L  # noqa: E402
from gsdf_amd import hip  # noqa: E402
from oracle.oracle import OracleSDF  # noqa: E402
from scaffold.builder import Builder  # noqa: E402


def main():
    assert os.environ.get("GSDF_HIP_FUSED_LEAF") == "1"
    hip.init(0)
    b = Builder()
    members = L.members(b)
    for name in ("spheres0", "boxeszero", "boxes-1e-13", "both_tiny"):
        sh, res = members[name]
        cpu = OracleSDF(sh.tree())
        want = L.sorted_bits(cpu.render_octree(res, 4096, True).tris)
        sdf = hip.SDF3HIP(sh)
        for kw in ({}, {"share_corners": 1}, {"prune": False}):
            oc = hip.OctreeHIP(sdf, res, **kw)
            got = L.sorted_bits(oc.RenderAll())
            assert got.shape == want.shape and (got == want).all(), (name, kw, got.shape, want.shape)
        print(name, sdf.info()["kernels"], len(want), "triangles")
        assert "leaf_kernel" in sdf.info()["kernels"]["leaf"]
    print("fused ok")


if __name__ == "__main__":
    main()
