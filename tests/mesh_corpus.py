"""The corpus as MESHES: every node type of tests/corpus.py in a tree that the meshers, their leaf kernels and the octree's
centre tests see (tests/test_mesh_corpus_ref.py on the host, tests/test_gpu_mesh_corpus.py on the device).

family(b) returns (name, shape):
  3-D corpus      every shapes3d() entry but the four scene_* (meshed by test_gpu_mesh.py, test_gpu_specialized.py, ...)
  ext_* / rev_*   every 2-D corpus shape and the Bezier shape under Extrude(s, 0.5) and under Revolve(s, 0): the only way a 2-D
                  op reaches a leaf kernel, a column brick or interval mode
  offseam_*       arrays whose repeated child sits OFF its cell or sector, so the field jumps across cell-centre planes and sector
                  rays (include/gsdf_seams.h): the six trees that lost surface to the centre tests, a twelve-sector one, and four
                  nestings of the first (Scale, Rotate about a general axis, Twist, operand of a Difference)
  circ_gated      a circular array behind the sector gate
  twoscrew_*      two unrotated screws that reach one column brick: the second overwrites the first's one-entry XYCache between the
                  brick's two passes

Resolution: float32(Diagonal / 40) -- six or seven octree levels, a brick, a level of centre tests
and a ragged last wave, 0.01 to 0.5 s of oracle time per tree. OMITTED names what is left out and why (at most MAX_OMITTED).
meshes() renders every tree once with the oracle and asserts the two caps."""
import functools

import numpy as np

import corpus
from gsdf_amd._ctypes_common import OPS
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32
DIV = 40
MAX_OMITTED = 6
NODE_TYPES = [o for o in OPS if o != "INVALID"]

# left out by name
OMITTED = {
    "ext_intersect2d": "the oracle's renderers refuse it: Intersection2D's Bounds() of the disjoint circle and rectangle is empty",
    "rev_intersect2d": "as ext_intersect2d (ext_ / rev_intersect2d_overlap hold the node type)",
    "rev_rotate2d2": "the oracle's renderers refuse it: the revolved outline's Bounds() comes out inverted",
    "offseam_circ12": "no surface at any resolution (the field's minimum over its bounds is +0.03: each sphere lies wholly in a sector "
                      "that does not evaluate it); its bounds are tested (bounds_only), offseam_circ12_r40 is meshed in its place",
}
# a parameter of their own: with the corpus's there is nothing to mesh at any resolution that a test can afford (Shell scales its
# child by the thickness, 1/128: a box of 0.008, and from 0.5 on it reaches past Bounds(); Offset2D by +0.33 of a rectangle 0.61 wide leaves nothing)
OWN_PARAMETER = {"shell": "Shell(a, 0.3) in the corpus's Difference", "ext_offset2d0": "Offset2D(obj, 0.2)", "rev_offset2d0": "Offset2D(obj, 0.2)"}
RES_DIV = {}   # name -> a divisor of its own (none needed with the parameters above)
# Bounds() is short upstream (the revolved circle off the axis; the polygon that closes itself), so the flat lattice and the octree
# see different parts of the surface: each renderer is compared with the oracle's own only
FLAT_DIFFERS = ("revolve_off", "ext_poly_selfclosed")
OFF_SEAM_DIVS = (47, 61, 83, 101)


def offseam_trees(b):
    s = b.NewSphere(0.25)
    base = b.Array(b.Translate(s, .9, 0, 0), .7, .7, .7, 3, 3, 3)
    out = [("offseam_array", base),
           ("offseam_array442", b.Array(b.Translate(b.NewSphere(.3), .5, .4, 0), .6, .6, .6, 4, 4, 2)),
           ("offseam_array_box", b.Array(b.Translate(b.NewBox(1, .61, .8, .3), 2, .3, 0), .7, .5, .6, 3, 2, 5)),
           ("offseam_circ", b.CircularArray(b.Translate(s, 1, .8, 0), 5, 7)),
           ("offseam_ext_circ2d", b.Extrude(b.CircularArray2D(b.Translate2D(b.NewCircle(.25), 1, .8), 6, 8), .5)),
           ("offseam_ext_array2d", b.Extrude(b.Array2D(b.Translate2D(b.NewCircle(.25), .5, .4), .6, .6, 4, 4), .5)),
           ("offseam_circ12", b.CircularArray(b.Translate(s, 1, .9, 0), 12, 12)),
           ("offseam_circ12_r40", b.CircularArray(b.Translate(b.NewSphere(0.4), 1, .9, 0), 12, 12)),
           ("offseam_scaled", b.Scale(base, 1.7)),
           ("offseam_rotated", b.Rotate(base, 0.7, (0.3, 1.0, 0.5))),
           ("offseam_twisted", b.Twist(base, 0.4)),
           ("offseam_cut", b.Difference(b.NewBox(3.2, 2.4, 2.4, 0.1), base))]
    return out


def twoscrew_trees(b):
    iso, npt = b.ScrewISO(1, .1, True, 2), b.ScrewNPT(.5, 1)
    return [("twoscrew_union", b.Union(iso, b.Translate(npt, 1.6, 0, 0))),
            ("twoscrew_translated", b.Union(b.Translate(iso, 0, 0, 0.25), b.Translate(npt, 1.6, 0, 0)))]


def gated_trees(b):
    """A circular array whose child costs enough for the sector gate (D_CIRC_ORDER, D_GATEOB: tests/test_lowering.py has the same
    tree) and is not its own mirror image in its sector's ray."""
    star = b.NewPolygon([(1.2 * np.cos(t) * (1 if i % 2 else 0.5), 1.2 * np.sin(t) * (1 if i % 2 else 0.5)) for i, t in enumerate(np.linspace(0, 2 * np.pi, 12, endpoint=False))])
    tooth = b.Translate(b.Rotate(b.Extrude(star, 3.0), 0.5, (0, 0, 1)), 6.0, 0, 0)
    return [("circ_gated", b.Union(b.NewCylinder(5.5, 2.0, 0.0), b.CircularArray(tooth, 9, 9)))]


def family(b=None, with_omitted=False):
    b = b or Builder()
    out = [(n, s) for n, s in corpus.shapes3d(b)[1] if not n.startswith("scene_")]
    a = b.NewBox(1, 0.61, 0.8, 0.3)   # corpus.shapes3d's box; "shell" as there, but 0.3 thick
    size = a.Bounds()[3:] - a.Bounds()[:3]
    half = b.Translate(b.Translate(b.NewBox(size[0] * 20, size[1] / 3, size[2] * 20, 0), 0, size[1] / 3, 0), 0, size[1] / 3, 0)
    out[[n for n, _ in out].index("shell")] = ("shell", b.Difference(b.Shell(a, 0.3), half))
    flat2d = corpus.shapes2d(b)[1] + corpus.bezier2d(b)[1]
    flat2d[[n for n, _ in flat2d].index("offset2d0")] = ("offset2d0", b.Offset2D(b.Translate2D(b.NewRectangle(1, 0.61), 2, .3), 0.2))
    # (the corpus's intersect2d is empty, see OMITTED: the same node over a circle that does reach the rectangle)
    flat2d.append(("intersect2d_overlap", b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 0.3), b.NewRectangle(1, 0.61))))
    for n, s in flat2d:
        out.append(("ext_" + n, b.Extrude(s, 0.5)))
        out.append(("rev_" + n, b.Revolve(s, 0)))
    out += offseam_trees(b) + twoscrew_trees(b) + gated_trees(b)
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    assert set(OMITTED) <= set(names) and len(OMITTED) <= MAX_OMITTED, sorted(set(OMITTED) - set(names))
    assert set(RES_DIV) | set(FLAT_DIFFERS) <= set(names) - set(OMITTED)
    return out if with_omitted else [(n, s) for n, s in out if n not in OMITTED]


NAMES = tuple(n for n, _ in family(Builder()))
CORPUS3D = tuple(n for n, _ in corpus.shapes3d(Builder())[1] if not n.startswith("scene_"))


def off_seam(name):
    return name.startswith("offseam_")


def bounds_only(b):
    """Trees whose bounds are tested although there is nothing to mesh."""
    return [(n, s) for n, s in family(b, with_omitted=True) if n == "offseam_circ12"]


def res_of(name, shape, div=None):
    return F(float(shape.Diagonal()) / (div or RES_DIV.get(name, DIV)))


def ops_of(shape):
    """Node types reachable from the shape's root (a builder's blob holds every node it ever made)."""
    t = shape.tree()
    seen, todo = set(), [t.root]
    while todo:
        i = todo.pop()
        if i not in seen:
            seen.add(i)
            nd = t.nodes[i]
            todo += [t.links[nd.link_off + k] for k in range(nd.nchild)]
    return {OPS[t.nodes[i].op] for i in seen}


def has_array(shape):
    return bool(ops_of(shape) & {"ARRAY", "ARRAY2D", "CIRCARRAY", "CIRCARRAY2D"})


@functools.lru_cache(maxsize=None)
def meshes():
    """{name: (shape, res, the oracle's default octree mesh)} of the family, rendered once per process and left unchanged. Asserts
    the caps: at most MAX_OMITTED trees left out, every node type in a tree meshed with more than 100 triangles."""
    b = Builder()
    out, seen = {}, set()
    for name, sh in family(b):
        res = res_of(name, sh)
        m = OracleSDF(sh.tree()).render_octree(res, 4096, True)
        out[name] = (sh, res, m)
        if m.n_tris > 100:
            seen |= ops_of(sh)
    assert len(OMITTED) <= MAX_OMITTED
    assert seen == set(NODE_TYPES), ("node types in no tree meshed with more than 100 triangles", sorted(set(NODE_TYPES) - seen))
    return out
