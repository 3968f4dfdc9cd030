"""tests/progcheck.py over every program family the suite builds, and over single corrupted words (no GPU).

  * every family is clean -- as built, without brick masks (GSDF_HIP_NO_BRICK_MASKS=1) and without the sector gate
    (GSDF_HIP_NO_SECTOR_GATE=1) -- and the walk saw what it is there for: every gate kind, a gate with an outer context, D_SKIP,
    D_UBOUND2D / 3D, D_CIRC_ORDER, D_LIP_SEAM, and a flagged D_FLAG_HXY consumer behind a skip target;
  * the checker has teeth: one word of a valid program changed, the violation reported at the changed instruction. These streams
    are checked only; nothing here is ever handed to a device;
  * the specialised build embeds the words of gsdf_hip_lower (kSpecCode of the generated source).

Measured: 3 s for the module on one CPU core (python -m pytest tests/test_progcheck.py -q), 1 208 programs in each of the three variants.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corpus
import fuzz_trees
import lattice_trees
import mesh_corpus
import nonlip_trees
import progcheck as PC
import scaled_corpus
import tree_edit
from degenerate_trees import degenerate_trees
from gsdf_amd import hip
from scaffold.builder import Builder
from test_scale_ref import RUNGS

with open(os.path.join(os.path.dirname(__file__), "golden", "iso-3098.ttf"), "rb") as _f:
    TTF = _f.read()
SCENES = ("npt-flange", "bolt", "knurled-cylinder", "fibonacci-showerhead", "glyph-plate")
POLY7 = [(0, 0), (2, 0), (2.5, 1), (2, 2), (1, 2.5), (0, 2), (-0.5, 1)]


def test_the_table_names_every_opcode():
    assert len(PC.NAMES) == len(PC.NPAR) and PC.NAMES[0] == "D_END"
    assert set(PC.TABLE) == set(PC.NAMES), (sorted(set(PC.NAMES) - set(PC.TABLE)), sorted(set(PC.TABLE) - set(PC.NAMES)))
    assert set(PC.GATES) == {n for n in PC.NAMES if n.startswith("D_GATE")} and set(PC.COMBINES) == {n for n in PC.NAMES if n.startswith("D_COMBINE")}


def hand_trees(b):
    """Trees for paths no family takes by itself (see the corruption tests below)."""
    ext = lambda: b.Extrude(b.NewPolygon(POLY7), 1.0)
    out = []
    # a gated child (the translated union: box region, expensive) that saves a position of its own; the enclosing intersection
    # reloads ITS position behind the gate's target (a gated child comes last in its own frame: the reload is the parent's)
    inner = b.Translate(b.Union(b.Translate(b.NewBox(1, 1, 1, 0), 1, 0, 0), ext()), 4, 0, 0)
    out.append(("load-behind-gate", b.Intersection(b.Union(b.NewTorus(1.0, 0.2), inner), b.Translate(b.NewSphere(3), 0, 0, 1))))
    # a gated child that refreshes the hypot register at another x,y, and a cylinder behind the gate's target
    prod = b.Translate(b.Intersection(b.NewCylinder(1, 2, 0), ext()), 4, 0, 0)
    # (z-only translate: the same x,y as in front of the gate, where the register was valid -- on the path that skips)
    out.append(("hypot-behind-gate", b.Intersection(b.Union(b.NewCylinder(3, 2, 0), prod), b.Translate(b.NewCylinder(8, 2, 0), 0, 0, 0.5))))
    # a rotation about y in front of a twist: P.z mixes the entry x
    out.append(("twist-behind-rotation", b.Rotate(b.Twist(b.NewBox(1, 0.5, 2, 0.05), 0.7), 0.4, (0, 1, 0))))
    # wide unions, 2-D and 3-D (tests/test_lowering.py)
    out.append(("wide3d", b.Union(b.NewSphere(1), b.Translate(b.NewBox(1, 1, 1, 0), 3, 0, 0), b.Translate(b.Extrude(b.NewRectangle(1, 1), 1), 6, 0, 0),
                                  b.Translate(b.NewTorus(1, 0.2), 9, 0, 0))))
    out.append(("wide2d", b.Union2D(b.NewCircle(1), b.Translate2D(b.NewCircle(1), 3, 0), b.Translate2D(b.NewCircle(1), 6, 0), b.Translate2D(b.NewCircle(1), 9, 0))))
    out.append(("x-translated-cylinders", b.Union(b.NewCylinder(1, 2, 0), b.Translate(b.NewCylinder(1, 2, 0), 0.5, 0, 0), b.Translate(b.NewCylinder(1, 2, 0), 0, 0, 3))))
    return out


def families():
    """name -> callable returning [(label, shape or tree)]; built under the environment of the calling test."""
    b = Builder()
    fam = {}
    fam["scenes"] = lambda: [(s, b.Scene(s)) for s in SCENES]
    fam["text-and-threads"] = lambda: [("text", b.Extrude(b.TextLine(TTF, "Abp8"), 0.2)), ("text2d", b.TextLine(TTF, "Ø12 äöü")),
                                       ("bolt-iso", b.BoltISO(3, 0.5, True, 2, 10.0, 2.0)), ("screw-buttress", b.ScrewPlasticButtress(1.6, 0.4, 1.2))]
    fam["corpus"] = lambda: corpus.shapes3d(b)[1] + corpus.shapes2d(b)[1] + corpus.bezier2d(b)[1]
    fam["fuzz3d"] = lambda: [(f"fuzz{seed}/{k}", s) for seed in (1, 2, 3, 4, 5, 6) for k, s in enumerate(fuzz_trees.random_shapes(seed, 14, depth=4)[1])] + \
                            [(f"fuzz11/{k}", s) for k, s in enumerate(fuzz_trees.random_shapes(11, 8, depth=3)[1])]
    fam["fuzz2d"] = lambda: [(f"fuzz2d{seed}/{k}", s) for seed, n in ((7, 24), (708, 6)) for k, s in enumerate(fuzz_trees.random_shapes2d(seed, n, depth=3)[1])]
    fam["nonlip"] = lambda: [(f"nonlip{seed}/{k}", s) for seed in (21, 22, 23) for k, s in enumerate(nonlip_trees.nonlip_shapes(seed, 12)[1])]
    fam["mesh_corpus"] = lambda: mesh_corpus.family(b, with_omitted=True)      # (the trees of mesh_corpus.meshes(), not their meshes)
    fam["lattice"] = lambda: [(n, sh) for n, (sh, _) in lattice_trees.members(b).items()]
    fam["scaled"] = lambda: [(f"{n}@2^{k}", s) for k in RUNGS for u in (scaled_corpus.unit(k),)
                             for n, s in scaled_corpus.shapes3d(b, u)[1] + scaled_corpus.shapes2d(b, u)[1] + scaled_corpus.bezier2d(b, u)[1]]
    fam["negative-scale"] = tree_edit.negative_scale_trees
    fam["degenerate"] = degenerate_trees
    fam["hand"] = lambda: hand_trees(b)
    return fam


FAMILIES = tuple(families())
VARIANTS = {"as-built": None, "no-brick-masks": "GSDF_HIP_NO_BRICK_MASKS", "no-sector-gate": "GSDF_HIP_NO_SECTOR_GATE"}
_seen = {}


def _clean(family, variant, monkeypatch):
    """Every program of the family under the variant's knob is clean; what the walks saw, summed (kept for the census below)."""
    if (family, variant) not in _seen:
        if VARIANTS[variant]:
            monkeypatch.setenv(VARIANTS[variant], "1")
        progs = families()[family]()
        assert progs
        t = {}
        for label, sh in progs:
            code, slots = hip.lower(sh)
            res = PC.check(code, slots)
            assert not res.violations, (family, label, variant, res.violations[:5])
            assert res.ins[-1].name == "D_END"
            for k, v in res.stats.items():
                t[k] = t.get(k, 0) + v
            if variant == "no-brick-masks":
                assert "D_SKIP" not in res.stats and "D_LIP_DOM" not in res.stats, (family, label)
            if variant == "no-sector-gate":
                assert "D_CIRC_ORDER" not in res.stats, (family, label)    # (a D_GATEOB may remain: a turned box under an ordinary combine)
        if VARIANTS[variant]:
            monkeypatch.delenv(VARIANTS[variant])
        _seen[(family, variant)] = t
    return _seen[(family, variant)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("family", FAMILIES)
def test_family_is_clean(family, variant, monkeypatch):
    _clean(family, variant, monkeypatch)


def test_the_families_reach_what_the_checker_is_for(monkeypatch):
    """What the clean programs contained, all families together (each family is walked once per module run, here or above)."""
    seen = {v: {} for v in VARIANTS}
    for v in VARIANTS:
        for fam in FAMILIES:
            for k, n in _clean(fam, v, monkeypatch).items():
                seen[v][k] = seen[v].get(k, 0) + n
    t = seen["as-built"]
    for name in ("D_GATE2D", "D_GATE3D", "D_GATEZC", "D_GATEOB", "D_SKIP", "D_UBOUND2D", "D_UBOUND3D", "D_CIRC_ORDER", "D_LIP_SEAM", "D_LIP_DOM",
                 "outer", "hxy_behind_target"):
        assert t.get(name, 0) >= 1, (name, t)
    # the families by themselves, without this module's hand trees, reach the same
    own = {}
    for fam in FAMILIES:
        if fam != "hand":
            for k, n in _clean(fam, "as-built", monkeypatch).items():
                own[k] = own.get(k, 0) + n
    assert all(own.get(name, 0) >= 1 for name in ("D_GATE2D", "D_GATE3D", "D_GATEZC", "D_GATEOB", "D_SKIP", "outer", "hxy_behind_target")), own
    # the knobs switch off what they say and nothing else
    assert seen["no-brick-masks"].get("D_GATE3D", 0) == t["D_GATE3D"] and seen["no-sector-gate"].get("D_SKIP", 0) == t["D_SKIP"]
    assert seen["no-sector-gate"].get("D_CIRC_ORDER", 0) == 0 and seen["no-brick-masks"].get("D_SKIP", 0) == 0


# ---------------------------------------------------------------------------------------------------- corruptions
def _prog(sh):
    code, slots = hip.lower(sh)
    res = PC.check(code, slots)
    assert not res.violations, res.violations[:5]
    return code, slots, res.ins


def _hit(code, slots, pc, what=None):
    """The corrupted stream is reported at the instruction that holds the corrupted word."""
    v = PC.check(code, slots).violations
    assert any(x.pc == pc and (what is None or what in x.what) for x in v), (pc, what, v[:6])


def _valid():
    b = Builder()
    out = {s: b.Scene(s) for s in ("npt-flange", "knurled-cylinder", "glyph-plate")}
    out["circ-gated"] = mesh_corpus.gated_trees(b)[0][1]
    out.update(dict(hand_trees(b)))
    return out


@pytest.fixture(scope="module")
def valid():
    return {k: _prog(sh) for k, sh in _valid().items()}


def _skipword(i):
    return i.pc + (3 if i.name == "D_SKIP" else 1 + PC.GATES[i.name] + 5)


def _span(ins, code, g):
    """Instructions of a gate's child: behind the gate, in front of its target."""
    t = g.pc + (int(code[_skipword(g)]) & 0xFFFFFF)
    return [i for i in ins if g.pc < i.pc < t], t


def test_skip_distances(valid):
    n = 0
    for name, (code, slots, ins) in valid.items():
        end = ins[-1].pc
        for i in ins:
            if i.name in PC.GATES or i.name == "D_SKIP":
                for delta in (1, -1):
                    c = code.copy()
                    c[_skipword(i)] = int(c[_skipword(i)]) + delta
                    _hit(c, slots, i.pc, "skip")
                c = code.copy()
                c[_skipword(i)] = (int(c[_skipword(i)]) & 0xFF000000) | (end - i.pc + 1)
                _hit(c, slots, i.pc, "beyond D_END")
                c[_skipword(i)] = (int(c[_skipword(i)]) & 0xFF000000) | (len(code) - i.pc + 7)
                _hit(c, slots, i.pc, "beyond D_END")
                c[_skipword(i)] = int(c[_skipword(i)]) & 0xFF000000
                _hit(c, slots, i.pc, "not forward")
                n += 1
    assert n >= 40


def test_gate_numbers_and_slots(valid):
    code, slots, ins = valid["npt-flange"]
    gates = [i for i in ins if i.name in PC.GATES]
    assert len(gates) == 2
    for g in gates:
        c = code.copy()
        c[_skipword(g)] += np.uint32(1 << 24)                      # the gate's brick-mask number changed
        _hit(c, slots, g.pc, "brick-mask number")
        c = code.copy()
        c[g.pc] = (int(c[g.pc]) & 0xFFFF) | ((g.slot + 1) << 16)   # the gate tests another slot than its combine uses
        _hit(c, slots, g.pc)
    sk = [i for i in ins if i.name == "D_SKIP"]
    c = code.copy()
    c[sk[1].pc + 1] = c[sk[0].pc + 1]                              # two D_SKIPs with one number
    _hit(c, slots, sk[1].pc, "brick-mask number")
    c = code.copy()
    c[sk[0].pc + 1] = 16
    _hit(c, slots, sk[0].pc, "not below 16")
    dom = [i for i in ins if i.name == "D_LIP_DOM"][0]
    c = code.copy()
    c[dom.pc + 1] = (int(c[dom.pc + 1]) + 1) % 6                   # kind of another combine
    _hit(c, slots, dom.pc)
    c = code.copy()
    c[dom.pc + 2] = 14                                             # a number no D_SKIP carries
    _hit(c, slots, dom.pc, "brick-mask number")


def test_hypot_flag(valid):
    # on a cylinder behind an x-translate
    code, slots, ins = valid["x-translated-cylinders"]
    n = 0
    for k, i in enumerate(ins):
        if i.name == "D_CYL0" and ins[k - 1].name == "D_TRANSLATE" and code.view(np.float32)[ins[k - 1].pc + 1] != 0:
            assert not i.word & PC.FLAG_HXY
            c = code.copy()
            c[i.pc] |= PC.FLAG_HXY
            _hit(c, slots, i.pc, "D_FLAG_HXY")
            n += 1
    assert n == 1
    # on the first consumer behind the target of a gate whose child holds a producer
    n = 0
    for name, (code, slots, ins) in valid.items():
        for g in ins:
            if g.name not in PC.GATES:
                continue
            span, t = _span(ins, code, g)
            if not any(PC.TABLE[i.name][4] == "ensure" and not i.word & PC.FLAG_HXY for i in span):
                continue
            behind = [i for i in ins if i.pc >= t and PC.TABLE[i.name][4] in ("ensure", "use")]
            if behind and not behind[0].word & PC.FLAG_HXY and not (behind[0].name == "D_GATEZC" and (code[behind[0].pc + 1] or code[behind[0].pc + 2])):
                c = code.copy()
                c[behind[0].pc] |= PC.FLAG_HXY
                _hit(c, slots, behind[0].pc, "D_FLAG_HXY")
                n += 1
    assert n >= 1
    # on an instruction that has no use for it
    code, slots, ins = valid["npt-flange"]
    sv = [i for i in ins if i.name == "D_SAVER"][0]
    c = code.copy()
    c[sv.pc] |= PC.FLAG_HXY
    _hit(c, slots, sv.pc, "does not take it")
    # D_SKIP promising a hypot its subtree does not leave
    # (flange: every subtree leaves the root's hypot, flagged or not; hypot-behind-gate: the gated subtree leaves another)
    n = {}
    for name in ("npt-flange", "hypot-behind-gate"):
        code, slots, ins = valid[name]
        for i in ins:
            if i.name == "D_SKIP" and not i.word & PC.FLAG_HXY:
                c = code.copy()
                c[i.pc] |= PC.FLAG_HXY
                v = PC.check(c, slots).violations
                assert all(x.pc == i.pc for x in v), v
                n[name] = n.get(name, 0) + bool(v)
    assert n["npt-flange"] == 0 and n["hypot-behind-gate"] >= 1, n


def test_slots(valid):
    # a D_LOADP3 pointed at a slot saved only inside a gated child
    n = 0
    for name, (code, slots, ins) in valid.items():
        for g in ins:
            if g.name not in PC.GATES:
                continue
            span, t = _span(ins, code, g)
            saves = [i for i in span if i.name == "D_SAVEP3"]
            loads = [i for i in ins if i.pc >= t and i.name == "D_LOADP3"]
            if saves and loads and loads[0].slot != saves[0].slot:
                c = code.copy()
                c[loads[0].pc] = (int(c[loads[0].pc]) & 0xFFFF) | (saves[0].slot << 16)
                _hit(c, slots, loads[0].pc, "column")
                n += 1
    assert n >= 1
    # a slot raised to lds_slots, on a write and on a read
    code, slots, ins = valid["npt-flange"]
    for kind in ("D_SAVER", "D_COMBINE_DIFF", "D_LOADP3", "D_SCREW_PRE", "D_MAXR_SLOT"):
        i = [j for j in ins if j.name == kind][0]
        c = code.copy()
        c[i.pc] = (int(c[i.pc]) & 0xFFFF) | (slots << 16)
        _hit(c, slots, i.pc, "lds_slots")
    # ... and the same program handed over with one slot less than it needs
    assert any("lds_slots" in v.what for v in PC.check(code, slots - 1).violations)
    # a combine that reads the slot of a value saved later
    code, slots, ins = valid["load-behind-gate"]
    sv = [i for i in ins if i.name == "D_SAVER"][0]
    c = code.copy()
    c[sv.pc] = (int(c[sv.pc]) & 0xFFFF) | ((sv.slot + 1) % slots << 16)
    assert PC.check(c, slots).violations


def test_dependency_flags(valid):
    code, slots, ins = valid["knurled-cylinder"]
    tw = [k for k, i in enumerate(ins) if i.name == "D_TWIST"]
    assert tw
    behind = [i for i in ins[tw[0] + 1:] if i.name == "D_CIRC_PRE"][0]
    assert not behind.word & PC.FLAG_SHXY
    c = code.copy()
    c[behind.pc] |= PC.FLAG_SHXY
    _hit(c, slots, behind.pc, "D_FLAG_SHXY")
    # a transform whose matrix mixes x into z, then a twist
    code, slots, ins = valid["twist-behind-rotation"]
    tr = [i for i in ins if i.name == "D_TRANSFORM"][0]
    assert code.view(np.float32)[tr.pc + 1 + 8] != 0
    tw = [i for i in ins if i.name == "D_TWIST"][0]
    assert tw.pc > tr.pc and not tw.word & PC.FLAG_SHZ
    c = code.copy()
    c[tw.pc] |= PC.FLAG_SHZ
    _hit(c, slots, tw.pc, "D_FLAG_SHZ")
    # the same twist without the x-z terms (the matrix of a rotation about z in their place) may carry it
    c = code.copy()
    f = c.view(np.float32)
    f[tr.pc + 1:tr.pc + 13] = np.array([[0.6, -0.8, 0, 0], [0.8, 0.6, 0, 0], [0, 0, 1, 0]], np.float32).reshape(-1)
    c[tw.pc] |= PC.FLAG_SHZ
    assert not PC.check(c, slots).violations


def test_interval_stack_and_tables(valid):
    code, slots, ins = valid["npt-flange"]
    pops = [i for i in ins if i.name == "D_LIP_POP"]
    assert len(pops) == 2
    for p in pops:
        for delta in (1, -1):
            if p.slot + delta < 0:
                continue
            c = code.copy()
            c[p.pc] = (int(c[p.pc]) & 0xFFFF) | ((p.slot + delta) << 16)
            _hit(c, slots, p.pc, "interval")
    push = [i for i in ins if i.name == "D_LIP_PUSH"][-1]
    c = code.copy()
    c[push.pc] = (int(c[push.pc]) & 0xFFFF) | ((push.slot + 1) << 16)
    _hit(c, slots, push.pc, "interval")
    # D_UBOUND*: a count raised by one runs over the next instruction; raised by many, beyond the code
    for name, kind in (("wide3d", "D_UBOUND3D"), ("wide2d", "D_UBOUND2D"), ("glyph-plate", "D_UBOUND2D")):
        code, slots, ins = valid[name]
        ub = [i for i in ins if i.name == kind][0]
        for more in (1, 1000):
            c = code.copy()
            c[ub.pc + 1] += np.uint32(more)
            _hit(c, slots, ub.pc)
    # D_CIRC_PRE: a table offset beyond the code, and one inside the instructions
    code, slots, ins = valid["knurled-cylinder"]
    cp = [i for i in ins if i.name == "D_CIRC_PRE"][0]
    assert ins[-1].pc < int(code[cp.pc + 4]) and int(code[cp.pc + 4]) + 2 * int(code.view(np.float32)[cp.pc + 2]) <= len(code)
    for tab in (len(code) - 1, len(code) + 64, ins[-1].pc - 8):
        c = code.copy()
        c[cp.pc + 4] = tab
        _hit(c, slots, cp.pc, "table")
    # a polygon whose vertex count runs beyond D_END; an opcode beyond the enum; no D_END
    code, slots, ins = valid["npt-flange"]
    po = [i for i in ins if i.name == "D_POLY2D"][0]
    c = code.copy()
    c[po.pc + 1] += np.uint32(4096)
    _hit(c, slots, po.pc)
    c = code.copy()
    c[ins[3].pc] = (int(c[ins[3].pc]) & ~0xFFF) | len(PC.NAMES)
    _hit(c, slots, ins[3].pc, "D_OP_COUNT")
    assert PC.check(code[:ins[-1].pc], slots).violations


# ---------------------------------------------------------------------------------------------------- the specialised build
@pytest.mark.parametrize("scene", ["npt-flange", "bolt", "knurled-cylinder"])
def test_specialised_source_embeds_the_lowered_words(scene):
    sh = Builder().Scene(scene)
    t = sh.tree()
    n = C.c_size_t()
    assert hip.lib().gsdf_hip_specialize_source(C.byref(t), None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value + 1)
    assert hip.lib().gsdf_hip_specialize_source(C.byref(t), buf, n.value + 1, C.byref(n)) == 0
    src = buf.value.decode()
    code, slots = hip.lower(sh)
    tab = re.search(r"kSpecCode\[(\d+)\] = \{(.*?)\};", src, re.S)
    assert int(tab.group(1)) == len(code)
    words = np.array([int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-f]+u", tab.group(2))], np.uint32)
    assert (words == code).all()
    # one block per instruction, at the checker's own instruction boundaries (D_END has none)
    res = PC.check(words, slots)
    assert not res.violations
    blocks = [(int(p), nm) for p, nm in re.findall(r"\{  // (\d+) (D_[A-Z0-9_]+)", src)]
    assert blocks == [(i.pc, i.name) for i in res.ins[:-1]]
