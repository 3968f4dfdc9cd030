#!/usr/bin/env python3
"""The reference's GLSL statement of every corpus shape, evaluated at fixed points -> tests/golden/glsl_reference_distances.npz.

    python tests/golden/make_glsl_golden.py <checkout of the reference>

tests/glslref renders, for a flattened tree, the GLSL program the reference's GPU path would compile (from the reference's own
AppendShaderBody methods and glbuild/glsllib, read from the checkout) and interprets it. This stores what that interpreter returns
at the points tests/test_glsl_crosscheck.py compares the oracle at -- positions and distances only, no reference source text -- so
that the comparison runs without the reference. Per shape: pos_<name> (float32, n x dim) and glsl_<name> (float64, n); n_bodies:
how many shader node structs of the reference have a body to render."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import corpus  # noqa: E402


def shapes():
    """(name, shader, dim) in the order the points are drawn: every 3-D shape, then the 2-D ones and the Bezier curves."""
    _, s3 = corpus.shapes3d()
    _, s2 = corpus.shapes2d()
    _, sz = corpus.bezier2d()
    return [(n, s, 3) for n, s in s3] + [(n, s, 2) for n, s in s2 + sz]


def points(rng, name, s, dim):
    """The test's points of one shape: uniform over 1.25 x its bounding box (+1e-3), 120 per shape (60 for the glyph plate)."""
    bb = s.Bounds().astype(np.float64)
    lo, hi = (bb[:3], bb[3:]) if dim == 3 else (bb[[0, 1]], bb[[3, 4]])
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 1.25 + 1e-3
    n = 60 if s.tree().n_nodes and name == "scene_glyph_plate" else 120
    return (c + (rng.random((n, dim)) * 2 - 1) * h).astype(np.float32)


def main(ref):
    from glslref.glsl import Interp
    from glslref.goshader import Reference
    r = Reference(ref)
    rng = np.random.default_rng(11)
    out = {"n_bodies": np.array(len(r.body))}
    for name, s, dim in shapes():
        tree = s.tree()
        src, root, _ = r.program(tree)
        prog = Interp(src)
        pos = points(rng, name, s, dim)
        out["pos_" + name] = pos
        out["glsl_" + name] = np.array([prog.call(root, [p.astype(np.float64)]) for p in pos], np.float64)
    np.savez_compressed(os.path.join(HERE, "glsl_reference_distances.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
