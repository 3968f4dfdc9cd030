"""Trees whose surfaces lie ON the meshing lattice: fields with exact zeros, -0.0 and |v| < 1e-12 at lattice points, so that every
marching path takes mcInterpolate's degenerate branches (marchcubes.go:100-115: a corner under 1e-12 snaps the vertex to it, two such
corners give t = 0.5, -0.0 is outside) -- which shapes with random or decimal parameters essentially never do.

The lattice is made dyadic through a carrier box of edge E = float32(1.9801980257034302): float32(1.01) * E == 2.0 exactly, so the
octree's origin (weldref.lattice_of: the bounds scaled by float32(1.01)) is exactly (-1, -1, -1), and with res = 2^-k every lattice
point is an exact dyadic float. Everything else is unioned in or cut out INSIDE the carrier and leaves the bounds alone.

census() is the CPU statement of which branches a member reaches; tests/test_lattice_ref.py holds the families to it, so that the
device tests (tests/test_gpu_lattice.py) cannot pass vacuously."""
import numpy as np

import weldref as W
from oracle.oracle import mc_tables

F32 = np.float32
E = F32(1.9801980257034302)
assert F32(F32(1.01) * E) == F32(2.0)
ORIGIN = (-1.0, -1.0, -1.0)
RADII = (0.25, 0.5, 1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -21)   # in units of res; the last two: one ulp-ish either side of a lattice point
BOX_VARIANTS = ("zero", "+1e-13", "-1e-13", "+2e-12")


def carrier(b):
    return b.NewBox(float(E), float(E), float(E), 0)


def shell(b):
    """The carrier hollowed out: its surface (at +-0.990099, between lattice planes) stays, the lattice inside is empty space."""
    return b.Difference(carrier(b), b.NewBox(1.75, 1.75, 1.75, 0))


def union_nested(b, parts, width=16):
    """Union of many parts as a tree of unions at most `width` wide (min is exact and associative: the same bits as one wide union)."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [b.Union(*parts[k:k + width]) if len(parts[k:k + width]) > 1 else parts[k] for k in range(0, len(parts), width)]
    return parts[0]


def spheres(b, seed, res_log2=3, block=13):
    """shell() united with spheres centred on lattice points, radii a few exact multiples of res: the centres are the block^3 points
    -0.75 + 0.125 c (every point with probability 0.45, default_rng(seed)); block = 13 is the family, a smaller block a reduced member
    for the tests that compile the tree at run time."""
    res = 2.0 ** -res_log2
    rng = np.random.default_rng(seed)
    c = np.stack(np.meshgrid(*[np.arange(block)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    keep = rng.random(len(c)) < 0.45
    rad = rng.choice(np.array(RADII), len(c)) * res
    balls = [b.Translate(b.NewSphere(float(r)), *[float(x) for x in (-0.75 + 0.125 * p)]) for p, r in zip(c[keep], rad[keep])]
    return b.Union(shell(b), union_nested(b, balls))


def _inner(b):
    return b.Union(b.NewBox(1, .5, .75, 0), b.Translate(b.NewSphere(.25), .5, .5, .5))


def boxes(b):
    """name -> carrier minus a box-and-sphere whose faces lie on lattice planes, plain ("zero": corners of exactly +0 and -0) and
    under offsets just under (+-1e-13) and just over (+2e-12) mcInterpolate's 1e-12."""
    out = {"zero": b.Difference(carrier(b), _inner(b))}
    for name, off in (("+1e-13", 1e-13), ("-1e-13", -1e-13), ("+2e-12", 2e-12)):
        out[name] = b.Difference(carrier(b), b.Offset(_inner(b), off))
    return out


def both_tiny(b):
    """Edges whose two ends are both under 1e-12 with opposite signs (t = 0.5): the carrier minus two boxes side by side, their faces
    z = +-0.25, y = +-0.25 coplanar on lattice planes. The first is plain: the difference's field -d is -0.0 on its faces (outside,
    tiny). The second is under Offset(+1e-13): its d there is -1e-13 and the field +1e-13 (outside, tiny) -- so far no sign change;
    the third, under Offset(-1e-13), gives -1e-13: INSIDE and tiny. Lattice edges in the face planes that cross a seam x = -0.25 or
    x = +0.25 between the third box and a neighbour run from a tiny inside corner to a tiny outside one."""
    left = b.Translate(b.NewBox(.5, .5, .5, 0), -.5, 0, 0)
    mid = b.Offset(b.NewBox(.5, .5, .5, 0), -1e-13)
    right = b.Translate(b.Offset(b.NewBox(.5, .5, .5, 0), 1e-13), .5, 0, 0)
    return b.Difference(carrier(b), b.Union(left, mid, right))


def members(b):
    """name -> (shape, res) of every family member the device tests mesh."""
    out = {f"spheres{s}": (spheres(b, s), F32(2.0 ** -3)) for s in range(4)}
    for n, sh in boxes(b).items():
        out["boxes" + n] = (sh, F32(2.0 ** -3))
    out["both_tiny"] = (both_tiny(b), F32(2.0 ** -3))
    out["boxeszero@5"] = (boxes(b)["zero"], F32(2.0 ** -5))
    return out


def all_leaves(levels):
    n = 1 << (levels - 1)
    return np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)


def zero_area(tris):
    """Triangles whose cross product (float32, as WriteBinarySTL forms it) is exactly (0, 0, 0)."""
    t = np.asarray(tris, F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        n = np.cross((t[:, 1] - t[:, 0]).astype(F32), (t[:, 2] - t[:, 0]).astype(F32))
    return (n == 0).all(axis=1)


def census(oracle_sdf, shape, res):
    """Which degenerate branches marching cubes takes on `shape` at `res`, over EVERY leaf of the lattice (vertices on lattice planes
    floor into the neighbouring leaf: weldref.leaves_of_triangles is no superset here). A dict:
      origin, levels; leaves (all), soup, keys (weldref.soup_of over them); cases: the set of cube cases of the cut leaves;
      slots: {'none', 'a', 'b', 'both'} triangle corners by which ends of their edge are under 1e-12; kind3: slots keyed as lattice points;
      corners: {'+0', '-0', 'tiny'} corner values of cut leaves; zero_area: triangles with a zero cross product."""
    res = F32(res)
    origin, levels = W.lattice_of(shape.Bounds(), res)
    leaves = all_leaves(levels)
    _, tri = mc_tables()
    d = oracle_sdf.Evaluate(W.leaf_corners(leaves, origin, res).reshape(-1, 3)).reshape(-1, 8)
    live = np.abs(d[:, 0]) <= F32(F32(2) * W.SQRT3) * res
    case = np.where(live, ((d < 0) * (1 << np.arange(8))).sum(axis=1), 0)
    cut = (case != 0) & (case != 255)
    ntri = (tri[case] >= 0).sum(axis=1) // 3
    leaf_of = np.repeat(np.arange(len(leaves)), 3 * ntri)
    first = np.cumsum(3 * ntri) - 3 * ntri
    within = np.arange(len(leaf_of)) - np.repeat(first, 3 * ntri)
    edge = tri[case[leaf_of], 3 * (within // 3) + (2 - within % 3)].astype(np.int64)
    v1, v2 = d[leaf_of, W.PAIR[edge, 0]], d[leaf_of, W.PAIR[edge, 1]]
    c1, c2 = np.abs(v1) < F32(1e-12), np.abs(v2) < F32(1e-12)
    soup, keys = W.soup_of(oracle_sdf, leaves, origin, res)
    dc = d[cut]
    return {"origin": origin, "levels": levels, "leaves": leaves, "soup": soup, "keys": keys,
            "cases": set(int(c) for c in np.unique(case[cut])),
            "slots": {"none": int((~c1 & ~c2).sum()), "a": int((c1 & ~c2).sum()), "b": int((c2 & ~c1).sum()), "both": int((c1 & c2).sum())},
            "kind3": int((keys >> np.uint64(60) == 3).sum()),
            "corners": {"+0": int(((dc == 0) & ~np.signbit(dc)).sum()), "-0": int(((dc == 0) & np.signbit(dc)).sum()),
                        "tiny": int(((dc != 0) & (np.abs(dc) < F32(1e-12))).sum())},
            "zero_area": int(zero_area(soup.reshape(-1, 3, 3)).sum())}


def sorted_bits(tris):
    """(n, 9) uint32: the triangles sorted by their bits (not by value: -0.0 and +0.0 are different triangles here)."""
    t = np.ascontiguousarray(tris, F32).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


def printable(c):
    return {k: (len(v) if k == "cases" else v) for k, v in c.items() if k not in ("leaves", "soup", "keys", "origin")}
