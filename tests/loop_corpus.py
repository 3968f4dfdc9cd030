"""Loop stacks that gsdf_hip_contour_create accepts and no slicer produces: what tests/test_loop_corpus_ref.py runs through the CPU
twins and tests/test_gpu_loop_corpus.py through the device -- loops on a small integer grid with repeated vertices, points, flattened
loops, bow-ties and repeated loops (grid_loops), hand cases of a few loops each (HAND), a stack of 300 layers most of which are empty
(tall_stack) and counts that are exact multiples of a wave, a workgroup, a tile or a batch (BOUNDARY; each proves its size with an
assert). Everything is built with contoursimpref.pack, so the keys are 7 v + 1. No GPU and no pytest here."""
import numpy as np

import contoursimpref as S
import hatchref as H
import offsetref as O
import skinref as K

F = np.float32

# ---- direction sets: raw (dx, dy), |dx|, |dy| <= 1, not both zero; on integer coordinates s, c_k and u_c are exact -------------------
AXIS = [(1.0, 0.0), (0.0, 1.0)]
DIAG = [(1.0, 1.0), (-1.0, 1.0), (0.5, 0.0)]
BACK = [(0.0, -1.0), (-1.0, 0.0), (-0.5, -0.5), (1.0, -1.0)]

# (spacing, directions, offset) of every hatch; (spacing, directions, below, above, offset) of every skin; (res, insets) of every offset
HATCHES = ((1.0, AXIS, 0.0), (0.5, DIAG, 0.5), (0.75, BACK, -0.25))
SKINS = ((1.0, AXIS, 1, 1, 0.0), (0.5, DIAG, 2, 0, 0.5), (0.5, DIAG, 0, 2, 0.5))
TALL_SKIN = (1.0, AXIS, 8, 8, 0.0)
OFFSETS = ((0.5, (0.0, 0.5, -1.0)), (1.0, (1.0,)))
EIGHT_INSETS = (0.5, (0.0, 0.25, 0.5, 1.0, -0.25, -0.5, -1.0, 1.5))
TILE_INSETS = (0.5, (0.0, 0.5, 1.5))     # the offset call of the two 'tiles' cases beside OFFSETS (no negative inset: the box does not grow)
SIMPLIFIES = ((0.0, 1), (1.0, 2))        # (tol, passes)


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def grid_loops(seed, n_loops=12, n_layers=3, G=8):
    """n_loops loops of 3 .. 8 vertices on the integer grid 0 .. G: one in six with a zero-length edge, one in six a single point, one
    in six flattened onto a horizontal line, one in six the loop before it again; the rest as drawn -- bow-ties, vertices on lattice
    nodes and hatch lines, collinear triples and shared vertices come by themselves on 9 x 9 points."""
    rng = np.random.default_rng(seed)
    loops = []
    for _ in range(n_loops):
        n = int(rng.integers(3, 9))
        l = rng.integers(0, G + 1, (n, 2)).astype(F)
        r = int(rng.integers(0, 6))
        if r == 0:
            l[1] = l[0]
        elif r == 1:
            l[:] = l[0]
        elif r == 2:
            l[:, 1] = l[0, 1]
        elif r == 3 and loops:
            l = loops[-1].copy()
        loops.append(l)
    layers = np.sort(rng.integers(0, n_layers, n_loops))
    return S.pack(loops, layers, n_layers)


SEEDS = range(64)
NEGATIVE_ZERO_SEEDS = range(16)


def negative_zeros(c, shift=4):
    """The stack moved by -shift (the grid 0 .. 8 becomes -4 .. 4) with every zero coordinate written as -0.0, which is as finite as
    any. Crossings at one place then differ in the sign bit of a zero by the edge they were computed from (x_a + t (x_b - x_a) is
    -0.0 only where both terms are), so which of the skin's records tied in u_c leads its group under (r, j) shows in the
    segments' bytes (tests/test_loop_corpus_ref.py asserts it on the twin's records). With positive zeros alone the tied records of
    this corpus have equal bytes and that order is invisible."""
    xy = (c.xy - F(shift)).astype(F)
    xy[xy == 0] = F(-0.0)
    return S.Loops(xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def box(x0, y0, x1, y1):
    """The rectangle (x0, y0) .. (x1, y1), counter-clockwise."""
    return np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], F)


POINT = np.array([(3, 2)] * 3, F)
COLLINEAR = np.array([(0, 0), (2, 1), (6, 3)], F)
BOWTIE = np.array([(0, 0), (4, 4), (4, 0), (0, 4)], F)
SQUARE = box(1, 1, 5, 5)
ON_LINES = box(1, 1, 4, 3)              # its horizontal sides lie on the lines y = 1 and y = 3 of direction (1, 0), spacing 1, offset 0
ON_NODES = box(1.5, 2, 4, 3.5)          # its vertices are nodes of the offset's lattice at res 0.5 (asserted in hand_cases)


def hand_cases():
    """name -> Loops. 'stack' holds every hand loop as a layer of one handle, so that the skin's windows see degenerate neighbours."""
    cases = {
        "point": S.pack([POINT]),
        "collinear": S.pack([COLLINEAR]),
        "bowtie": S.pack([BOWTIE]),
        "doubled": S.pack([SQUARE, SQUARE]),
        "reversed": S.pack([SQUARE, SQUARE[::-1].copy()]),
        "shared vertex": S.pack([box(0, 0, 2, 2), box(2, 2, 4, 4)]),
        "shared edge": S.pack([box(0, 0, 2, 2), box(2, 0, 4, 2)]),
        "on lines": S.pack([ON_LINES]),
        "on nodes": S.pack([ON_NODES]),
        "stack": S.pack([POINT, COLLINEAR, BOWTIE, SQUARE, SQUARE, SQUARE, SQUARE[::-1].copy(), box(0, 0, 2, 2), box(2, 2, 4, 4), box(0, 0, 2, 2),
                         box(2, 0, 4, 2), ON_LINES, ON_NODES], [0, 1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8], 9),
    }
    # the claims of the names
    assert (np.diff(POINT, axis=0) == 0).all()
    d = np.diff(COLLINEAR.astype(np.float64), axis=0)
    assert d[0, 0] * d[1, 1] == d[0, 1] * d[1, 0]
    assert float(S.measures(cases["bowtie"])[0][0]["area"]) == 0.0
    s, off = 1.0, 0.0
    assert all((y - off) / s == int((y - off) / s) for y in ON_LINES[:, 1].tolist())
    for res, insets in OFFSETS[:1] + (EIGHT_INSETS,):
        _, _, xs, ys, _ = O.lattice(cases["on nodes"], res, insets)
        assert all(x in xs.tolist() and y in ys.tolist() for x, y in ON_NODES.tolist())
    return cases


# ---- 300 layers, eight of them occupied ------------------------------------------------------------------------------------------------
TALL_LAYERS = 300
TALL_OCCUPIED = (0, 63, 64, 65, 255, 256, 257, 299)
TALL_EMPTY_READ = (1, 254)               # the two empty layers whose D lattice the device test reads as well


def tall_stack():
    """One small square in each of the layers 0, 63, 64, 65, 255, 256, 257 and 299 -- either side of the first wave's and the first
    workgroup's last lane in every kernel that runs a layer per lane -- and nothing in the other 292. Half sides and centres differ
    between neighbouring layers, so that with a window of 1 layer 64 carries inner and top pieces and layer 256 inner and bottom ones."""
    half = (2.0, 3.0, 2.0, 1.5, 1.5, 2.0, 3.0, 1.0)
    cx = (4.0, 4.0, 4.5, 4.0, 3.0, 3.5, 3.5, 4.0)
    cy = (4.0, 4.0, 4.0, 3.5, 4.0, 4.0, 4.5, 4.0)
    c = S.pack([K.square(a, x, y) for a, x, y in zip(half, cx, cy)], list(TALL_OCCUPIED), TALL_LAYERS)
    assert c.n_layers == 300 and sorted(set(c.loop_layer.tolist())) == list(TALL_OCCUPIED) and len(c.loop_layer) == 8
    return c


# ---- boundary sizes ------------------------------------------------------------------------------------------------------------------
def edges_per_layer(c):
    return np.bincount(np.repeat(c.loop_layer, np.diff(c.loop_start.astype(np.int64))), minlength=c.n_layers).tolist()


def boundary_cases():
    """name -> Loops, each with the assert that it has the size its name claims."""
    cases = {}
    # a layer of exactly one and of exactly two batches of 256 edges: the offset's batch loop ends with a full batch
    for n in (256, 512):
        c = cases["circle %d" % n] = S.pack([S.circle(n)])
        assert edges_per_layer(c) == [n]
    # lattices of whole tiles only, and of one node more than whole tiles (pinned: nx = floor(fl(fl(hi - lo) / res)) + 4 at insets >= 0)
    c = cases["tiles 32 x 32"] = S.pack([box(0, 0, 14, 14), box(3, 3, 6, 9)[::-1].copy()])
    nx, ny = O.lattice(c, *TILE_INSETS)[:2]
    assert (nx, ny) == (32, 32) and nx % 16 == 0 and ny % 16 == 0
    c = cases["tiles 33 x 17"] = S.pack([box(0, 0, 14.5, 6.5), box(3, 3, 6, 5)[::-1].copy()])
    nx, ny = O.lattice(c, *TILE_INSETS)[:2]
    assert (nx, ny) == (33, 17) and nx % 16 == 1 and ny % 16 == 1
    # line buckets of exactly a wave and exactly a workgroup of records; three layers of them for the skin
    for teeth in (32, 128):
        c = cases["comb %d" % teeth] = H.comb(teeth)
        assert H.hatch(c, *HATCHES[0]).stats["max_line_crossings"] == 2 * teeth
        c = cases["combs %d" % teeth] = K.shifted_combs(teeth)
        assert K.skin(c, 1.0, [(1.0, 0.0)], 1, 1).stats["max_line_crossings"] == 6 * teeth
    # exactly a workgroup of vertices; one more, in a last loop whose closing edge returns from workgroup 1 to workgroup 0
    c = cases["256 vertices"] = S.pack([S.circle(100, 4.0, 4.0, 4.0), S.circle(150, 3.0, 4.5, 4.0), S.circle(6, 2.0, 4.0, 4.5)])
    assert len(c.xy) == 256
    c = cases["257 vertices"] = S.pack([S.circle(100, 4.0, 4.0, 4.0), S.circle(150, 3.0, 4.5, 4.0), S.circle(7, 2.0, 4.0, 4.5)])
    assert len(c.xy) == 257 and (int(c.loop_start[-2]), int(c.loop_start[-1]) - 1) == (250, 256)
    return cases


# ---- the twins, every one on one stack ---------------------------------------------------------------------------------------------------
def run_twins(c, tall=False, hand=False):
    """Every twin call of the device test on one stack: a dict of results by (consumer, arguments)."""
    import massref as M
    out = {"measures": S.measures(c), "sections": M.sections(c.xy, c.loop_start, c.loop_layer, c.n_layers)}
    for tol, passes in SIMPLIFIES:
        out["simplify", tol, passes] = S.simplify(c, F(tol), 8, passes)
    for k, (sp, dirs, off) in enumerate(HATCHES):
        out["hatch", k] = H.hatch(c, sp, dirs, off)
    for k, (sp, dirs, below, above, off) in enumerate(SKINS + ((TALL_SKIN,) if tall else ())):
        out["skin", k] = K.skin(c, sp, dirs, below, above, off)
    for k, (res, insets) in enumerate(OFFSETS + ((EIGHT_INSETS,) if hand else ())):
        out["offset", k] = O.offset(c, res, insets)
    return out
