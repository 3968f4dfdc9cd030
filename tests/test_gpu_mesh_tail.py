"""The end of the evaluating kernels' wave pass (leaf_block_tail: lane-invariant leaf words, scalar bookkeeping, the mirrored exchange
layout of leaf_eval_kernel) and the marching kernels behind it, through every route that reaches them, against the oracle, bit for
bit.

Shapes: a sphere and npt-flange at Diagonal / 24, / 40 (five and six levels: a few dozen bricks, blocks with and without cut leaves)
and / 300 (nine levels: leaf coordinates above 255, thousands of blocks) -- all of them meshes of three levels or more, whose wave
pass is one level-3 brick -- and at Diagonal / 2.5, the two-level lattice of eight leaves that takes the leaf-per-lane form of
leaf_eval_kernel with its run-time shift (asserted below: Diagonal / 24 has five levels, not fewer than three; the sphere's eight
leaves are all cut, of npt-flange's eight none is -- an empty mesh through every route). Routes: interpreter and specialised kernels x
share_corners 0, 1, 2 (leaf_eval_kernel, leaf_dense_kernel, the distinct-rows form) x triangles payload (march_records_kernel) and
records payload (pack + march_dense_kernel).

What the oracle is asked for:
  triangles, n_tris  OracleSDF.render_octree: the sorted triangles must be equal bit for bit.
  evals              render_octree's own counts: every corner of every surviving leaf (share_corners = 0), 64 columns x the distinct z
                     rows of each surviving brick (2), the distinct lattice points in passes of 256 lane slots or with the specialised
                     build's tail passes (1). Meshes of fewer than three levels have no bricks: every option evaluates every corner.
  cut_leaves         render_octree reports none. The leaves under its triangles (weldref.leaves_of_triangles: a superset of the leaves
                     that made them) are marched again with the oracle's distances (marchCubes' rule: |d0| <= 2 sqrt3 res, case not 0
                     or 255); the test first proves that this reproduces render_octree's triangle set exactly, so the leaves that cut
                     are the oracle's cut leaves -- every cut leaf emits a triangle, and none was pruned away.
  active_leaves      leaves of the surviving cubes with |d0| <= 2 sqrt3 res. render_octree does not name its survivors, so its
                     level-synchronous descent (oracle/orc_render.c: the centre of every cube of level >= 3 through
                     OracleSDF.EvaluateBounds with maxDist = size sqrt3 / 2, pruned when lo >= 0 or hi <= 0) is walked again here with
                     the oracle's evaluator; the walk proves itself against render_octree's own `pruned` and `evals`, and the
                     oracle's |d0| test is counted over the leaves it leaves. Every route must report exactly that count; and with
                     prune=False, where every leaf of the lattice survives, the count over the whole lattice (the three small sizes:
                     at most 2^15 leaves).
  which kernels ran  a specialised handle on a mesh of three levels or more must name specialised kernels for the leaf phase and,
                     once used, for share_corners 1 and 2 (both build without scratch for these two trees): a build that fell back
                     would otherwise be held to the fallback's counts. The library names a handle's kernels, not a mesh's: on the
                     two-level lattice what can be observed is that the handle never built or used a brick kernel and that every
                     option evaluated every corner of every leaf -- the leaf-per-lane form.
"""
import numpy as np
import pytest

import weldref as W
from lattice_trees import all_leaves, sorted_bits
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

F32 = np.float32
SCENES = ("sphere", "npt-flange")
DIVS = (2.5, 24, 40, 300)
FULL_LATTICE_MAX_LEVELS = 7   # (2^18 leaves: the oracle walks the whole lattice in a fraction of a second)
_b = Builder()
_ref = {}


def shape_of(scene):
    return _b.NewSphere(1.0) if scene == "sphere" else _b.Scene(scene)


class Ref:
    """The oracle's answers for one shape at one size, made once and left unchanged."""

    def __init__(self, scene, div):
        self.shape = shape_of(scene)
        self.res = F32(float(self.shape.Diagonal()) / div)
        self.cpu = OracleSDF(self.shape.tree())
        m = self.cpu.render_octree(self.res, 4096, True)
        self.levels, self.n_tris, self.tris = m.levels, m.n_tris, sorted_bits(m.tris)
        self.evals, self.evals_rows, self.pruned = m.evals, m.evals_rows, m.pruned
        self.evals_points_256, self.evals_points_tails = m.evals_points_256, m.evals_points_tails
        self.origin, levels = W.lattice_of(self.shape.Bounds(), self.res)
        assert levels == self.levels and (self.levels < 3) == (div == 2.5) and (self.n_tris > 0 or (scene, div) == ("npt-flange", 2.5))
        # cut leaves: the leaves under the oracle's triangles, marched again from the oracle's distances
        self.cut_leaves = 0
        if self.n_tris:
            cand = W.leaves_of_triangles(m.tris, self.origin, self.res)
            live, cut = self.classify(cand)
            soup, _ = W.soup_of(self.cpu, cand, self.origin, self.res)
            assert (sorted_bits(soup.reshape(-1, 9)) == self.tris).all(), "the candidate leaves do not reproduce the oracle's triangles"
            self.cut_leaves = int(cut.sum())
        # active leaves: marchCubes' first-corner test over the leaves the oracle's descent leaves
        self.leaves = self.walk()
        self.active_leaves = int(self.live(self.leaves).sum())
        assert self.cut_leaves <= self.active_leaves <= len(self.leaves)
        # active leaves without pruning: every leaf of the lattice
        self.full_active = None
        if self.levels <= FULL_LATTICE_MAX_LEVELS:
            live, cut = self.classify(all_leaves(self.levels))
            self.full_active = int(live.sum())
            assert int(cut.sum()) == self.cut_leaves    # (pruning loses no cut leaf of these shapes)

    def walk(self):
        """The leaves that survive the oracle's centre tests, in leaf units (orc_render.c, orc_render_octree: every cube of level >= 3
        is tested at its centre against the field's bounds over the ball of radius size sqrt3 / 2), proved against the `pruned` and
        `evals` render_octree itself reports."""
        corner = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.int64)
        cur = np.zeros((1, 3), np.int64)
        pruned = evals = 0
        for level in range(self.levels, 1, -1):
            if level >= 3:
                size = F32(F32(1 << (level - 1)) * self.res)
                max_dist = F32(size * F32(W.SQRT3 / F32(2)))
                o = (self.origin[None, :] + size * (cur >> (level - 1)).astype(F32)).astype(F32)
                centre = (F32(0.5) * (o + (o + size).astype(F32)).astype(F32)).astype(F32)
                lo, hi = self.cpu.EvaluateBounds(centre, max_dist)
                evals += len(cur)
                prunable = (lo >= 0) | (hi <= 0)
                pruned += int(prunable.sum()) << (3 * (level - 1))
                cur = cur[~prunable]
            if len(cur) == 0:
                break
            cur = (cur[:, None, :] + corner[None, :, :] * (1 << (level - 2))).reshape(-1, 3)
        else:
            evals += 8 * len(cur)
        assert (pruned, evals) == (self.pruned, self.evals), ("the walk is not the oracle's", pruned, self.pruned, evals, self.evals)
        return cur

    def live(self, leaves):
        o = (self.origin[None, :] + self.res * np.asarray(leaves).astype(F32)).astype(F32)   # corner 0, as weldref.leaf_corners forms it
        return np.abs(self.cpu.Evaluate(o)) <= F32(F32(2) * W.SQRT3) * self.res   # marchCubes' first-corner test

    def classify(self, leaves):
        d = self.cpu.Evaluate(W.leaf_corners(leaves, self.origin, self.res).reshape(-1, 3)).reshape(-1, 8)
        live = np.abs(d[:, 0]) <= F32(F32(2) * W.SQRT3) * self.res   # marchCubes' first-corner test
        case = ((d < 0) * (1 << np.arange(8))).sum(axis=1)
        return live, live & (case != 0) & (case != 255)


def ref(scene, div):
    if (scene, div) not in _ref:
        _ref[(scene, div)] = Ref(scene, div)
    return _ref[(scene, div)]


def leaf_evals(R, sdf, sc, leaf_cubes):
    """The oracle's count of the leaf phase's evaluations under share_corners = sc, for the kernels the handle has just used."""
    info = sdf.info()
    kern = info["kernels"]
    bricks = R.levels >= 3 and info["leaf_k"] == 4     # (a wave pass is a level-3 brick, evaluated four points per lane)
    if sc == 2 and bricks and (kern.get("leaf_rows") or not kern.get("leaf", "").endswith(":specialised")):
        return R.evals_rows   # (a specialised handle whose distinct-rows build needs scratch keeps every row)
    if sc == 1 and bricks:
        return R.evals_points_tails if kern.get("leaf_dense") else R.evals_points_256
    return 8 * leaf_cubes


def check(gpu, scene, div, specialised):
    R = ref(scene, div)
    sdf = gpu.SDF3HIP(R.shape)
    if specialised:
        sdf.specialize()
    for sc in (0, 1, 2):
        for payload in ("triangles", "records"):
            what = (scene, div, "specialised" if specialised else "interpreter", sc, payload)
            if payload == "records":
                oc = gpu.OctreeHIP(sdf, R.res, share_corners=sc, payload=gpu.PAYLOAD_RECORDS)
                assert tuple(oc.payload()[:2]) == (gpu.PAYLOAD_RECORDS, R.cut_leaves), (what, oc.payload())
                oc.march()
            else:
                oc = gpu.OctreeHIP(sdf, R.res, share_corners=sc)
            st = oc.stats
            print(what, "levels", st.levels, "tris", oc.n_tris(), "cut", int(st.cut_leaves), "active", int(st.active_leaves),
                  "evals", int(st.evals), "leaf evals", int(st.evals_leaf), "kernels", sdf.info()["kernels"])
            assert st.levels == R.levels and tuple(st.origin[:]) == tuple(R.origin) and st.res == R.res, what
            kern = sdf.info()["kernels"]
            assert kern["leaf"].startswith("leaf_eval_kernel<"), (what, kern)
            if R.levels < 3:     # no brick kernel was built or used: the leaf-per-lane form
                assert "leaf_dense" not in kern and "leaf_rows" not in kern, (what, kern)
            elif specialised:    # the kernels built for the tree ran, not a fallback
                assert kern["leaf"].endswith(":specialised"), (what, kern)
                assert sc != 1 or kern.get("leaf_dense", "").endswith(":specialised"), (what, kern)
                assert sc != 2 or kern.get("leaf_rows", "").endswith(":specialised"), (what, kern)
            else:
                assert kern["leaf"].endswith(":interpreter"), (what, kern)
            got = sorted_bits(oc.RenderAll())
            assert got.shape == R.tris.shape and (got == R.tris).all(), what
            assert oc.n_tris() == R.n_tris and int(st.n_tris) == R.n_tris, what
            assert int(st.cut_leaves) == R.cut_leaves, (what, int(st.cut_leaves), R.cut_leaves)
            assert int(st.active_leaves) == R.active_leaves, (what, int(st.active_leaves), R.active_leaves)
            assert int(st.leaf_cubes) == len(R.leaves), (what, int(st.leaf_cubes), len(R.leaves))
            want_leaf = leaf_evals(R, sdf, sc, int(st.leaf_cubes))
            assert int(st.evals_leaf) == want_leaf, (what, int(st.evals_leaf), want_leaf)
            assert int(st.evals) - int(st.evals_leaf) == R.evals - 8 * int(st.leaf_cubes), what   # the centre tests: the oracle's
            if sc == 0:
                assert int(st.evals) == R.evals, (what, int(st.evals), R.evals)
            if R.full_active is not None:   # every leaf of the lattice survives: the oracle's |d0| test at each of them
                full = gpu.OctreeHIP(sdf, R.res, share_corners=sc, prune=False,
                                     **({"payload": gpu.PAYLOAD_RECORDS} if payload == "records" else {}))
                if payload == "records":
                    full.march()
                assert int(full.stats.active_leaves) == R.full_active, (what, int(full.stats.active_leaves), R.full_active)
                assert int(full.stats.cut_leaves) == R.cut_leaves and (sorted_bits(full.RenderAll()) == R.tris).all(), what


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("scene", SCENES)
def test_interpreter_routes_match_the_oracle(gpu, scene, div):
    check(gpu, scene, div, specialised=False)


@pytest.mark.parametrize("div", DIVS)
@pytest.mark.parametrize("scene", SCENES)
def test_specialised_routes_match_the_oracle(gpu, scene, div):
    check(gpu, scene, div, specialised=True)
