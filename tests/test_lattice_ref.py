"""The lattice-aligned families (tests/lattice_trees.py) held to what they are for, from the oracle and the numpy twin alone: the
lattice is dyadic, the degenerate branches of mcInterpolate are reached in numbers, and twin, oracle octree and oracle flat renderer
agree bit for bit on every member -- the conditions under which tests/test_gpu_lattice.py cannot pass vacuously, and under which a
device mismatch there is the device's."""
import numpy as np
import pytest

import lattice_trees as L
import weldref as W
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

_cache = {}


def member(name):
    """(shape, res, oracle, census) of a family member, computed once."""
    if name not in _cache:
        if "b" not in _cache:
            _cache["b"] = Builder()
            _cache["members"] = L.members(_cache["b"])
        sh, res = _cache["members"][name]
        cpu = OracleSDF(sh.tree())
        c = L.census(cpu, sh, res)
        print(name, L.printable(c))
        _cache[name] = (sh, res, cpu, c)
    return _cache[name]


NAMES = [f"spheres{s}" for s in range(4)] + ["boxes" + v for v in L.BOX_VARIANTS] + ["both_tiny", "boxeszero@5"]


def test_names_are_the_members():
    assert sorted(NAMES) == sorted(L.members(Builder()))


def test_lattice_is_dyadic():
    b = Builder()
    bb = L.carrier(b).Bounds()
    assert (np.abs(bb) == L.E / np.float32(2)).all()
    for sh in (L.shell(b), L.spheres(b, 0), L.boxes(b)["zero"], L.boxes(b)["+2e-12"], L.both_tiny(b)):
        assert (sh.Bounds().view(np.uint32) == bb.view(np.uint32)).all()      # nothing inside the carrier moves the bounds
        for k, levels in ((3, 5), (4, 6)):
            origin, lv = W.lattice_of(sh.Bounds(), np.float32(2.0 ** -k))
            assert (origin == np.float32(-1)).all() and lv == levels
            m = OracleSDF(sh.tree()).render_octree(np.float32(2.0 ** -k), 4096, True)
            assert m.levels == levels
    # every lattice point is then the exact dyadic float, and a leaf's two copies of a plane agree
    pos = W.leaf_corners(L.all_leaves(5), np.float32([-1, -1, -1]), np.float32(0.125))
    assert (pos * 8 == np.rint(pos * 8)).all() and pos.min() == -1 and pos.max() == 1


def test_spheres_reach_every_case_and_snap_in_numbers():
    cases = set()
    for s in range(4):
        _, _, _, c = member(f"spheres{s}")
        cases |= c["cases"]
        assert c["kind3"] >= 10000 and c["zero_area"] >= 1500, L.printable(c)
        assert c["kind3"] == c["slots"]["a"] + c["slots"]["b"]
    assert cases == set(range(1, 255))


def test_every_snap_class_is_reached():
    for v in ("zero", "+1e-13", "-1e-13"):
        c = member("boxes" + v)[3]
        assert c["slots"]["a"] >= 32 and c["slots"]["b"] >= 32 and c["slots"]["none"] >= 32, L.printable(c)
    assert member("boxeszero")[3]["corners"]["-0"] >= 1000
    assert member("boxes+1e-13")[3]["corners"]["tiny"] >= 32 and member("boxes-1e-13")[3]["corners"]["tiny"] >= 32
    c = member("both_tiny")[3]
    assert c["slots"]["both"] >= 32 and c["slots"]["a"] >= 32 and c["slots"]["b"] >= 32, L.printable(c)
    # the control just above the threshold: the same cut, nothing snapped
    c = member("boxes+2e-12")[3]
    assert c["slots"]["a"] == c["slots"]["b"] == c["slots"]["both"] == c["kind3"] == 0 and c["slots"]["none"] > 0
    assert c["corners"] == {"+0": 0, "-0": 0, "tiny": 0}
    # the reduced member the device tests specialise: still snapped and degenerate throughout
    b = Builder()
    sh = L.spheres(b, 0, block=7)
    c = L.census(OracleSDF(sh.tree()), sh, np.float32(0.125))
    print("spheres0 block 7", L.printable(c))
    assert c["kind3"] >= 1000 and c["zero_area"] >= 100 and len(c["cases"]) >= 128


@pytest.mark.parametrize("name", NAMES)
def test_twin_equals_octree_equals_flat(name):
    sh, res, cpu, c = member(name)
    soup = L.sorted_bits(c["soup"])
    nop = cpu.render_octree(res, 4096, False)
    assert nop.levels == c["levels"] and nop.n_tris == len(soup) > 0
    assert (soup == L.sorted_bits(nop.tris)).all()
    oc = cpu.render_octree(res, 4096, True)
    if name != "boxeszero@5":
        assert oc.pruned == 0            # five levels: no level is centre-tested
        assert oc.n_tris == len(soup) and (soup == L.sorted_bits(oc.tris)).all()
    else:
        # Seven levels: the centre tests run, and |d| TIES the threshold (octreerenderer.go:273, `>=`: a tie prunes). The cubes of edge
        # 4 res that touch a corner of the cut-out box with one of their own corners have their centre exactly half a diagonal from
        # it; their one cut leaf holds a triangle with all three corners snapped to that lattice point. So pruning drops point
        # triangles here and nothing else -- the reference's behaviour, and what the device's TotalPruned() must reproduce.
        assert oc.pruned > 0 and 0 < len(soup) - oc.n_tris <= 8
        have = set(map(bytes, L.sorted_bits(oc.tris)))
        gone = np.array([np.frombuffer(t, np.float32) for t in set(map(bytes, soup)) - have]).reshape(-1, 3, 3)
        assert len(gone) == len(soup) - oc.n_tris and (gone == gone[:, :1]).all()
        assert have <= set(map(bytes, soup))
        same = cpu.render_octree(res, 4096, True, assume_sdf=True)
        assert (L.sorted_bits(same.tris) == L.sorted_bits(oc.tris)).all() and same.pruned == oc.pruned
    fl = cpu.render_flat(res, 4096, 2)
    assert fl.n_tris == len(soup) and (soup == L.sorted_bits(fl.tris)).all()
