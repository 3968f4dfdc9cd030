"""Lift a shape to a chosen LDS slot count (host-only helper of tests/test_variant_census.py and tests/test_gpu_variants.py).

The interpreter kernels exist in several template instantiations and a handle picks one from its tree's slot count
(gsdf_amd/csrc/abi_program.h: batch_k, sweep_waves, leaf_config). lift() wraps a shape as the innermost operand of a right-nested
chain op(pad_i, rest): the pad's value waits in a slot of its own while `rest` is evaluated, so every link adds exactly one slot
(measured, 3-D and 2-D alike, with the pad as the FIRST operand of Xor / Difference / SmoothDifference / Xor2D / Difference2D; with
the shape first, or under Union, the count stays put). What the shape's own ops compute is unchanged: the same nodes see the same
positions.

The pads are chosen so that the shape's value still reaches the output over most of the sampled region -- a chain that hid it would
run the shape's ops without checking them:
  Xor / Xor2D        a small box / rectangle (sphere / circle every other time) inside the shape's bounds: the field changes around
                     the pad and equals the chain below elsewhere;
  Difference(2D),    a box / rectangle larger than the sampled region, translated a little: inside it the link negates the chain
  SmoothDifference   below (max(pad, -rest), pad deeply negative)
                     (1.3 x the bounds: corpus.sample_points reaches 25 % past them), so the chain below still decides the output
                     wherever it is smaller in magnitude than the distance to the pad's faces.
The ops rotate link by link (Xor, Difference, SmoothDifference in 3-D; Xor2D, Difference2D in 2-D: there is no smooth 2-D difference).

The first translated pad costs the slots of the position it saves, so a chain cannot reach every count just above the shape's own:
lift() then tries the link without its Translate, and raises if the target cannot be hit exactly.
"""
import math

import numpy as np

import corpus
from gsdf_amd import hip
from gsdf_amd._ctypes_common import OPS

# Both sides of every selection boundary and one tree well inside K = 1. The sweeps run four workgroups per CU while
# 4 * (slots * K KB + 64) fits 160 KB (sweep_waves): up to 9 slots at K = 4 and up to 19 at K = 2 -- one below the 10 and 20 a
# bare 160 KB / 4 would give, hence the rungs 9 and 19 beside 10 | 11 and 20 | 21; K goes 4 -> 2 at 12 | 13 and 2 -> 1 at 28 | 29
# (batch_k), and the leaf phase's K goes 4 -> 2 at 11 | 12 already (leaf_config).
RUNGS = (9, 10, 11, 12, 13, 19, 20, 21, 28, 29, 40)
# slot classes by the eval sweep's (K, W): (name, lowest, highest slot count), and the rungs inside each
CLASSES = (("K4W4", 0, 9), ("K4W3", 10, 12), ("K2W4", 13, 19), ("K2W3", 20, 28), ("K1", 29, 1 << 30))
CLASS_RUNGS = ((9,), (10, 11, 12), (13, 19), (20, 21, 28), (29, 40))

_GOLD = 0.6180339887498949
_steps = {}


def slots(shape):
    return hip.lower(shape)[1]


def class_of(nslots):
    return next(i for i, (_, lo, hi) in enumerate(CLASSES) if lo <= nslots <= hi)


def _frac(i, a):
    return (0.5 + (i + 1) * _GOLD * (a + 1) * 0.7548776662466927) % 1.0


def _link(b, rest, i, lo, hi, translate):
    """One link over `rest`: op(pad_i, rest). lo / hi: the ORIGINAL shape's bounds (the chain's own grow link by link)."""
    dim = len(lo)
    size = hi - lo
    ctr = (lo + hi) / 2
    m = float(size.min())
    if dim == 3:
        kind = i % 3
        if kind == 0:    # Xor with a small pad inside the bounds
            at = lo + size * (0.2 + 0.6 * np.array([_frac(i, a) for a in range(3)]))
            pad = b.NewSphere(0.09 * m) if (i // 3) % 2 else b.NewBox(0.15 * m, 0.11 * m, 0.13 * m, 0)
            if translate:
                pad = b.Translate(pad, *[float(np.float32(v)) for v in at])
            return b.Xor(pad, rest)
        pad = b.NewBox(*[float(np.float32(1.3 * s)) for s in size], 0)
        if translate:
            pad = b.Translate(pad, *[float(np.float32(c + 0.02 * s * (_frac(i, a) - 0.5))) for a, (c, s) in enumerate(zip(ctr, size))])
        return b.Difference(pad, rest) if kind == 1 else b.SmoothDifference(float(np.float32(0.05 * m)), pad, rest)
    if i % 2 == 0:
        at = lo + size * (0.2 + 0.6 * np.array([_frac(i, a) for a in range(2)]))
        pad = b.NewCircle(0.09 * m) if (i // 2) % 2 else b.NewRectangle(0.15 * m, 0.11 * m)
        if translate:
            pad = b.Translate2D(pad, *[float(np.float32(v)) for v in at])
        return b.Xor2D(pad, rest)
    pad = b.NewRectangle(*[float(np.float32(1.3 * s)) for s in size])
    if translate:
        pad = b.Translate2D(pad, *[float(np.float32(c + 0.02 * s * (_frac(i, a) - 0.5))) for a, (c, s) in enumerate(zip(ctr, size))])
    return b.Difference2D(pad, rest)


def lift(builder, shape, nslots):
    """`shape` as the innermost operand of a right-nested chain of binary ops whose lowering reports exactly `nslots` slots."""
    have = slots(shape)
    if nslots < have:
        raise ValueError(f"the shape has {have} slots of its own: it cannot be lifted down to {nslots}")
    bb = np.asarray(shape.Bounds(), np.float64)
    dim = 2 if shape.is2d else 3
    lo, hi = np.minimum(bb[:3][:dim], bb[3:][:dim]), np.maximum(bb[:3][:dim], bb[3:][:dim])
    if (hi - lo).min() < 0.1 * (hi - lo).max() or not (hi - lo).max() > 0:   # (an intersection's bounds may be empty or inverted: pads need a size)
        half = np.maximum((hi - lo) / 2, 0.05 * max(float((hi - lo).max()), 1.0))
        lo, hi = (lo + hi) / 2 - half, (lo + hi) / 2 + half
    # the chain of translated pads is the same for every target: keep its steps per shape (a lift to 40 slots passes all lower rungs)
    steps = _steps.setdefault((id(builder), shape.id), (builder, [(have, shape)]))[1]   # (the builder is kept with its steps: its id stays its own)
    have, cur = max((s for s in steps if s[0] <= nslots), key=lambda s: s[0])
    i = steps.index((have, cur))
    on_main = True
    while have < nslots:
        for translate in (True, False):
            nxt = _link(builder, cur, i, lo, hi, translate)
            n = slots(nxt)
            if have < n <= nslots:
                break
        else:
            raise ValueError(f"no link takes {have} slots to at most {nslots} (link {i} gives {n})")
        cur, have, i = nxt, n, i + 1
        on_main = on_main and translate
        if on_main and i == len(steps):
            steps.append((have, cur))
    return cur


def ops_of(shape):
    t = shape.tree()
    return {OPS[t.nodes[i].op] for i in range(t.n_nodes)}


# ---- the trees of tests/test_gpu_variants.py (lowered and counted, host-only, by tests/test_variant_census.py)

def eval_cases(b, dim, cls):
    """Part (a): every corpus shape of dimension `dim` (2: the bezier shape included) lifted to one rung of slot class `cls`; which
    rung of the class rotates from shape to shape. (name, rung, lifted shape), lazily."""
    shapes = corpus.shapes3d(b)[1] if dim == 3 else corpus.shapes2d(b)[1] + corpus.bezier2d(b)[1]
    for k, (name, sh) in enumerate(shapes):
        rungs = [r for r in CLASS_RUNGS[cls] if r >= slots(sh)]
        if rungs:
            rung = rungs[k % len(rungs)]
            yield name, rung, lift(b, sh, rung)


MESH_RUNGS = (12, 13, 19, 20, 21, 28, 29, 40)
MESH_BASES = ("screw_iso_ext", "circarray0", "twist", "smoothunion", "extrude_polygon", "revolve_off")
IMAGE_BASES = ("poly", "circarray2d0", "xor2d", "translatemulti")


def mesh_bases(b):
    """Part (b): a screw, a circular array, a twist (interval mode in the centre tests), a smooth blend, an extrusion of a polygon and
    a revolution."""
    d = dict(corpus.shapes3d(b)[1])
    star = [(math.cos(2 * math.pi * i / 10) * (1.0 if i % 2 else 0.55), math.sin(2 * math.pi * i / 10) * (1.0 if i % 2 else 0.55)) for i in range(10)]
    d["extrude_polygon"] = b.Extrude(b.NewPolygon(star), 0.6)
    return [(n, d[n]) for n in MESH_BASES]


def image_bases(b):
    d = dict(corpus.shapes2d(b)[1])
    return [(n, d[n]) for n in IMAGE_BASES]
