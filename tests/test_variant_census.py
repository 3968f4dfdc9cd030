"""Which interpreter kernel variant do the suite's trees reach? Host-only: every tree is lowered (gsdf_hip_lower) and classed by its
LDS slot count, from which a handle picks K (points per lane) and W (workgroups per CU): abi_program.h: batch_k, sweep_waves.

Trees per slot class, as printed by test_family_table (pytest -s):

  family                            <=9 K4W4  10-12 K4W3  13-19 K2W4  20-28 K2W3      >28 K1
  corpus 3-D                              40           1           0           0           0
  corpus 2-D                              44           0           0           0           0
  corpus bezier                            1           0           0           0           0
  scenes                                   4           1           0           0           0
  fuzz 3-D (seeds 1-6)                    50          25           9           0           0
  fuzz 2-D                                24           0           0           0           0
  fuzz dual contouring                     8           0           0           0           0
  non-Lipschitz (21-23)                   35           1           0           0           0
  lattice members                         10           0           0           0           0
  degenerate trees                         9           0           0           0           0
  negative-scale trees                     6           0           0           0           0
  text plate                               1           0           0           0           0
  32-sphere union                          1           0           0           0           0
  (so far: 270 trees, 37 above nine slots, 9 above twelve, none above nineteen, no 2-D tree above nine; from here on: the lifted
   trees of slot_ladder.py)
  lifted corpus 3-D (variants a)          40          41          41          41          41
  lifted corpus 2-D + bezier              45          45          45          45          45
  lifted mesh bases (variants b)           0           6          12          18          12
  lifted image bases (variants b)          0           4           8          12           8

(The classes are the code's: four workgroups per CU need 4 * (slots * K KB + 64 B) <= 160 KB, so W drops to 3 at ten slots for
K = 4 and at twenty for K = 2, a slot earlier than 160 KB / 4 alone would put it.)

and every node type (all of _ctypes_common.OPS but INVALID) occurs in a lifted tree of every class: test_every_op_in_every_class.
"""
import os

import numpy as np
import pytest

import corpus
import fuzz_trees
import lattice_trees
import slot_ladder as SL
from gsdf_amd._ctypes_common import OPS
from nonlip_trees import nonlip_shapes
from scaffold.builder import Builder
from test_gpu_nan import degenerate_trees
from tree_edit import negative_scale_trees

SCENES = ["npt-flange", "bolt", "knurled-cylinder", "glyph-plate", "fibonacci-showerhead"]


@pytest.fixture(scope="module")
def bld():
    return Builder()


def test_one_slot_per_link_in_both_dimensions(bld):
    """The ladder's step: a link op(Translate(pad), rest) adds exactly one slot once the chain holds a translated pad, for every op
    the ladder uses, in 3-D and in 2-D; with the operands the other way round the count stays put."""
    for base in (bld.NewSphere(1), bld.NewCircle(1)):
        counts = [SL.slots(SL.lift(bld, base, n)) for n in range(6, 30)]
        assert counts == list(range(6, 30))
    sphere = bld.NewSphere(1)      # ... up to the largest tree a handle is made for, and one more (include/gsdf_hip.h: "Largest trees")
    assert [SL.slots(SL.lift(bld, sphere, n)) for n in (52, 53, 67, 68, 80, 81, 143, 144)] == [52, 53, 67, 68, 80, 81, 143, 144]
    for base, pad, xor in ((bld.NewSphere(1), lambda i: bld.Translate(bld.NewBox(.1, .1, .1, 0), .1 * i, 0, 0), bld.Xor),
                           (bld.NewCircle(1), lambda i: bld.Translate2D(bld.NewRectangle(.1, .1), .1 * i, 0), bld.Xor2D)):
        cur, counts = base, []
        for i in range(6):
            cur = xor(cur, pad(i))          # the chain as the FIRST operand: nothing waits while the pad is evaluated
            counts.append(SL.slots(cur))
        assert len(set(counts[1:])) == 1, counts


def test_lift_refuses_what_it_cannot_reach(bld):
    knurled = dict(corpus.shapes3d(bld)[1])["scene_knurled_cylinder"]
    assert SL.slots(knurled) == 10 and SL.lift(bld, knurled, 10) is knurled and SL.slots(SL.lift(bld, knurled, 11)) == 11
    with pytest.raises(ValueError):
        SL.lift(bld, knurled, 9)


@pytest.mark.parametrize("dim", [3, 2])
def test_every_rung_reached_exactly(bld, dim):
    """Every tree of test_gpu_variants.py's part (a) lowers to exactly its rung, and all eleven rungs occur for the dimension."""
    seen = set()
    for cls in range(len(SL.CLASSES)):
        n = 0
        for name, rung, sh in SL.eval_cases(bld, dim, cls):
            assert SL.slots(sh) == rung and SL.class_of(rung) == cls and sh.is2d == (dim == 2), (name, rung, SL.slots(sh))
            seen.add(rung)
            n += 1
        assert n == (41 if dim == 3 else 45) - (1 if (dim, cls) == (3, 0) else 0), (dim, cls, n)   # (knurled-cylinder has ten slots of its own)
    assert seen == set(SL.RUNGS)


def test_mesh_and_image_bases_reach_their_rungs(bld):
    for name, sh in SL.mesh_bases(bld) + SL.image_bases(bld):
        for rung in SL.MESH_RUNGS:
            assert SL.slots(SL.lift(bld, sh, rung)) == rung, (name, rung)
    ops = set().union(*[SL.ops_of(sh) for _, sh in SL.mesh_bases(bld)])
    assert {"SCREW", "CIRCARRAY", "TWIST", "SMOOTH_UNION", "EXTRUSION", "POLY2D", "REVOLUTION"} <= ops


def test_every_op_in_every_class(bld):
    """Every node type occurs in at least one lifted tree of every slot class: the share left out is zero. A node type the corpus
    gains later fails here until test_gpu_variants.py runs it under every variant too."""
    want = set(OPS) - {"INVALID"}
    for cls, (cname, _, _) in enumerate(SL.CLASSES):
        have = set()
        for dim in (3, 2):
            for _, _, sh in SL.eval_cases(bld, dim, cls):
                have |= SL.ops_of(sh)
        assert have >= want, (cname, sorted(want - have))


def _families(b):
    yield "corpus 3-D", [s for _, s in corpus.shapes3d(b)[1]]
    yield "corpus 2-D", [s for _, s in corpus.shapes2d(b)[1]]
    yield "corpus bezier", [s for _, s in corpus.bezier2d(b)[1]]
    yield "scenes", [b.Scene(n) for n in SCENES]
    yield "fuzz 3-D (seeds 1-6)", [s for seed in range(1, 7) for s in fuzz_trees.random_shapes(seed, 14, depth=4)[1]]
    yield "fuzz 2-D", fuzz_trees.random_shapes2d(7, 24, depth=3)[1]
    yield "fuzz dual contouring", fuzz_trees.random_shapes(11, 8, depth=3)[1]
    yield "non-Lipschitz (21-23)", [s for seed in (21, 22, 23) for s in nonlip_shapes(seed, 12)[1]]
    yield "lattice members", [sh for sh, _ in lattice_trees.members(b).values()]
    yield "degenerate trees", [t for _, t in degenerate_trees()]
    yield "negative-scale trees", [t for _, t in negative_scale_trees()]
    ttf = open(os.path.join(os.path.dirname(__file__), "golden", "iso-3098.ttf"), "rb").read()   # (test_gpu_mesh.py: _text_plate)
    t2 = b.TextLine(ttf, "gsdf MI355X")
    bb = t2.Bounds()
    plate = b.Translate(b.NewBox(float(bb[3] - bb[0]) + 0.3, float(bb[4] - bb[1]) + 0.3, 0.06, 0.01), float(bb[0] + bb[3]) / 2, float(bb[1] + bb[4]) / 2, -0.08)
    yield "text plate", [b.Union(b.Extrude(t2, 0.12), plate)]
    rng = np.random.default_rng(9)
    yield "32-sphere union", [b.Union(*[b.Translate(b.NewSphere(0.2 + 0.1 * i / 32), *(rng.random(3) * 4 - 2)) for i in range(32)])]
    for dim, label in ((3, "lifted corpus 3-D (variants a)"), (2, "lifted corpus 2-D + bezier")):
        yield label, [sh for cls in range(len(SL.CLASSES)) for _, _, sh in SL.eval_cases(b, dim, cls)]
    yield "lifted mesh bases (variants b)", [SL.lift(b, sh, r) for _, sh in SL.mesh_bases(b) for r in SL.MESH_RUNGS]
    yield "lifted image bases (variants b)", [SL.lift(b, sh, r) for _, sh in SL.image_bases(b) for r in SL.MESH_RUNGS]


def test_family_table(bld):
    """The family x class table of the module docstring, printed; the unlifted families stay below 21 slots (which is why the
    variants needed trees of their own), the lifted ones fill every class."""
    rows = {}
    print("\n  %-30s" % "family" + "".join("%12s" % ("%s %s" % (("<=%d" % hi) if lo == 0 else (">%d" % (lo - 1)) if hi > 1000 else ("%d-%d" % (lo, hi)), n))
                                         for n, lo, hi in SL.CLASSES))
    for fam, shapes in _families(bld):
        row = [0] * len(SL.CLASSES)
        for sh in shapes:
            row[SL.class_of(SL.slots(sh))] += 1
        rows[fam] = row
        print("  %-30s" % fam + "".join("%12d" % v for v in row))
    for fam in ("corpus 3-D", "corpus 2-D", "corpus bezier", "scenes", "fuzz 2-D", "fuzz dual contouring", "non-Lipschitz (21-23)", "lattice members", "degenerate trees", "negative-scale trees", "text plate", "32-sphere union"):
        assert sum(rows[fam][2:]) == 0, (fam, rows[fam])      # (nothing above twelve slots)
    assert rows["fuzz 3-D (seeds 1-6)"][4] == 0 and sum(rows["fuzz 3-D (seeds 1-6)"][2:]) <= 9
    assert rows["lifted corpus 3-D (variants a)"] == [40, 41, 41, 41, 41] and rows["lifted corpus 2-D + bezier"] == [45] * 5
    assert rows["lifted mesh bases (variants b)"] == [0, 6, 12, 18, 12] and rows["lifted image bases (variants b)"] == [0, 4, 8, 12, 8]
