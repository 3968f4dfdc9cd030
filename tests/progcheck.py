"""A checker of lowered device programs (gsdf_amd/csrc/dev_ops.h) over ALL of their paths, on the CPU.

Every kernel executes the word stream of gsdf_hip_lower unchecked: the program counter advances by word counts read from the stream,
skip distances, LDS slot numbers, box counts and table offsets are taken as given, and several promises the stream makes (the cached
hypot of D_FLAG_HXY, the coordinate dependencies of D_FLAG_SHXY / D_FLAG_SHZ, "this slot was written on every path that gets here")
are tracked by the host compiler alone. check(code, lds_slots) decodes the stream and walks it once -- every branch is a forward
skip, so the state that a taken skip carries waits at its target and meets the fall-through state there -- and returns what breaks
a rule as Violation(pc, instruction name, text).

TABLE below is written from the cases of interp.h (what each instruction reads and writes there), not from compile.cpp: the checker
must not restate the code it checks. Per opcode: reads / writes over {x, y, z, R}, the LDS columns [slot, slot + n) it reads and
writes, its use of D_FLAG_HXY and how it maps the dependencies of P on the entry coordinates. Lengths are kDevOpParams of dev_ops.h
plus the four variable forms.

The interval stack, as interp.h and the lowering use it: D_LIP_PUSH stores at the level its slot names, a D_LIP_POP restores from
one. The push at the entry of a combine frame is never popped -- D_LIP_DOM reads it by number (pinfo) and the next push at that
level overwrites it -- so the rule is: a push names a level <= the current depth (no gaps), a pop names a live level whose entry
no D_LIP_DOM has named (a map's own push), and every entry that a push or pop drops unpopped was named by a D_LIP_DOM (a frame's).
"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "gsdf_amd", "csrc", "dev_ops.h")) as _f:
    _HDR = _f.read()
_ENUM = _HDR[_HDR.index("enum DevOp"):_HDR.index("D_OP_COUNT")]
NAMES = [n for n in dict.fromkeys(re.findall(r"\b(D_[A-Z0-9_]+)\b", re.sub(r"//[^\n]*", "", _ENUM)))]
NPAR = [int(x) for x in re.findall(r"\*/\s*(\d+)", re.search(r"kDevOpParams\[D_OP_COUNT\] = \{(.*?)\};", _HDR, re.S).group(1))]
FLAG_SHZ, FLAG_SHXY, FLAG_HXY, FLAG_SWAP, OP_MASK = 0x1000, 0x2000, 0x4000, 0x8000, 0x0FFF

Violation = namedtuple("Violation", "pc name what")
Ins = namedtuple("Ins", "pc name word slot n")   # n = words of the instruction, its own word included

# name -> (reads, writes, columns read, columns written, hxy, dep)
#   reads / writes : over "xyzR" (what the case's statements touch of P and R)
#   hxy            : "ensure" -- ENSURE_HXY(): with the flag the register is read, without it written for the current x,y;
#                    "use"    -- read with the flag, never written (D_GATEZC); "skip" -- D_SKIP: written on the TAKEN path with the flag
#   dep            : how the dependencies of P.x / P.y / P.z on the entry coordinates change (resolved in check())
_P3, _P2 = ("xyz", "R", 0, 0, None, None), ("xy", "R", 0, 0, None, None)
_POST = ("R", "R", 0, 0, None, None)
_COMB = ("R", "R", 1, 0, None, None)
_GATE = ("xyz", "", 1, 0, None, None)
TABLE = {
    "D_END": ("R", "", 0, 0, None, None),
    "D_SPHERE": _P3, "D_BOX": _P3, "D_BOXFRAME": _P3, "D_HEX": _P3,
    "D_TORUS": ("xyz", "R", 0, 0, "ensure", None), "D_CYL0": ("xyz", "R", 0, 0, "ensure", None), "D_CYLR": ("xyz", "R", 0, 0, "ensure", None),
    "D_LINE2D": _P2, "D_ARC2D": _P2, "D_QUADBEZIER2D": _P2, "D_EQTRI2D": _P2, "D_RECT2D": _P2, "D_DIAMOND2D": _P2, "D_X2D": _P2,
    "D_HEX2D": _P2, "D_OCT2D": _P2, "D_ELLIPSE2D": _P2, "D_POLY2D": _P2, "D_LINES2D": _P2,
    "D_CIRCLE2D": ("xy", "R", 0, 0, "ensure", None),
    "D_TRANSLATE": ("xyz", "xyz", 0, 0, None, "componentwise"),      # (writes narrowed by tx, ty, tz: x - 0.0f is x, bit for bit)
    "D_SCALE_PRE": ("xyz", "xyz", 0, 0, None, "componentwise"),
    "D_SYMMETRY": ("xyz", "xyz", 0, 0, None, "componentwise"),       # (writes narrowed by the bits)
    "D_TRANSFORM": ("xyz", "xyz", 0, 0, None, "matrix3"),
    "D_TWIST": ("xyz", "xy", 0, 0, None, "twist"),
    "D_ROT2D": ("xy", "xy", 0, 0, None, "matrix2"),
    "D_EXTRUDE_PRE": ("z", "", 0, 1, None, None),
    "D_REVOLVE_PRE": ("xz", "x", 0, 0, None, "revolve"),
    "D_SCREW_PRE": ("xyz", "xy", 0, 1, "ensure", "screw"),
    "D_ELONGATE_PRE": ("xyz", "xyz", 0, 1, None, "componentwise"),
    "D_ELONGATE2D_PRE": ("xy", "xy", 0, 1, None, "componentwise"),
    "D_ARRAY_PRE": ("", "xyz", 3, 0, None, "columns3"),
    "D_ARRAY2D_PRE": ("", "xy", 2, 0, None, "columns2"),
    "D_CIRC_PRE": ("xy", "xy", 0, 2, None, "circ"),
    "D_LOADP2_SUB": ("", "xy", 2, 0, None, "columns2"),
    "D_MULR": _POST, "D_SHELL_POST": _POST, "D_ADDR": _POST, "D_ANNULUS": _POST,
    "D_EXTRUDE_POST": _COMB, "D_MAXR_SLOT": _COMB, "D_ADDR_SLOT": _COMB,
    "D_SAVEP3": ("xyz", "", 0, 3, None, None), "D_LOADP3": ("", "xyz", 3, 0, None, "load"),
    "D_SAVEP2": ("xy", "", 0, 2, None, None), "D_LOADP2": ("", "xy", 2, 0, None, "load"),
    "D_SAVER": ("R", "", 0, 1, None, None), "D_SETSLOT": ("", "", 0, 1, None, None), "D_SETR": ("", "R", 0, 0, None, None),
    "D_COMBINE_MIN": _COMB, "D_COMBINE_MAX": _COMB, "D_COMBINE_DIFF": _COMB, "D_COMBINE_XOR": _COMB,
    "D_COMBINE_SUNION": _COMB, "D_COMBINE_SDIFF": _COMB, "D_COMBINE_SINTER": _COMB,
    "D_GATE2D": ("xy", "", 1, 0, None, None), "D_GATE3D": _GATE, "D_GATEZC": ("xyz", "", 1, 0, "use", None), "D_GATEOB": _GATE,
    "D_UBOUND2D": ("xy", "", 0, 1, None, None), "D_UBOUND3D": ("xyz", "", 0, 1, None, None),
    "D_CIRC_ORDER": ("xy", "xy", 2, 2, None, "circ"),
    "D_LIP_PUSH": ("xyz", "", 0, 0, None, None), "D_LIP_POP": ("", "", 0, 0, None, None), "D_LIP_MUL": ("", "", 0, 0, None, None),
    "D_LIP_WRAP": ("x", "", 0, 0, None, None),
    "D_SKIP": ("", "", 0, 0, "skip", None),
    "D_LIP_DOM": ("R", "", 1, 0, None, None),
    "D_LIP_SEAM": ("xyz", "", 0, 0, None, None),                     # (bit 3: reads columns slot, slot + 1)
}
GATES = {"D_GATE2D": 4, "D_GATE3D": 6, "D_GATEZC": 7, "D_GATEOB": 8}   # name -> index of the `sg` parameter (GSDF_GATE_TEST's I0)
COMBINES = ("D_COMBINE_MIN", "D_COMBINE_MAX", "D_COMBINE_DIFF", "D_COMBINE_XOR", "D_COMBINE_SUNION", "D_COMBINE_SDIFF", "D_COMBINE_SINTER")
DOM_KIND = {"D_COMBINE_MIN": 0, "D_COMBINE_MAX": 1, "D_COMBINE_DIFF": 2, "D_COMBINE_SUNION": 3, "D_COMBINE_SDIFF": 4, "D_COMBINE_SINTER": 5}
SWAP_TAKERS = COMBINES + ("D_LIP_DOM",)


def _length(code, pc, name, end):
    """Words of the instruction at pc (None: a variable form that does not fit in front of `end`)."""
    n = NPAR[NAMES.index(name)]
    if pc + 1 + n > end:
        return None
    if name == "D_POLY2D":
        nv = int(code[pc + 1]) & 0x7FFFFFFF
        n = ((pc + 4 + 7) & ~7) - (pc + 1) + 8 * nv
    elif name == "D_LINES2D":
        n = 2 + 5 * int(code[pc + 1])
    elif name in ("D_UBOUND2D", "D_UBOUND3D"):
        n = 1 + (4 if name == "D_UBOUND2D" else 6) * int(code[pc + 1])
    return 1 + n if pc + 1 + n <= end else None


def decode(code):
    """([Ins], [Violation]): the stream instruction by instruction up to its D_END (or to the first word that cannot be decoded)."""
    ins, bad, pc = [], [], 0
    while True:
        if pc >= len(code):
            bad.append(Violation(pc, "-", "the stream ends without D_END"))
            break
        w = int(code[pc])
        op = w & OP_MASK
        if op >= len(NAMES):
            bad.append(Violation(pc, "-", f"opcode {op} is not below D_OP_COUNT"))
            break
        name = NAMES[op]
        n = _length(code, pc, name, len(code))
        if n is None:
            bad.append(Violation(pc, name, "the instruction runs past the end of the code"))
            break
        if name in ("D_UBOUND2D", "D_UBOUND3D"):   # (here, not in the walk: a count that runs over other words derails the decoding behind it)
            d = 2 if name == "D_UBOUND2D" else 3
            box = np.asarray(code[pc + 2:pc + n], np.uint32).view(np.float32).reshape(-1, 2 * d).astype(np.float64)
            tiny = (box != 0) & (np.abs(box) < np.finfo(np.float32).tiny)
            if not np.isfinite(box).all() or tiny.any() or (box[:, :d] > box[:, d:]).any():
                bad.append(Violation(pc, name, "a listed box is not a box (corners not finite, subnormal or out of order): the count runs over other words"))
        ins.append(Ins(pc, name, w, w >> 16, n))
        if name == "D_END":
            break
        pc += n
    return ins, bad


def _mix(dep, row):
    """Dependencies of one output coordinate of a linear map: those of the inputs its row does not multiply by zero."""
    out = 0
    for d, m in zip(dep, row):
        if m != 0:
            out |= d
    return out


class _State:
    __slots__ = ("xy", "z", "hxy", "cols", "R", "dep", "lip")

    def copy(self):
        s = _State()
        s.xy, s.z, s.hxy, s.cols, s.R, s.dep, s.lip = self.xy, self.z, self.hxy, dict(self.cols), self.R, list(self.dep), self.lip
        return s


Result = namedtuple("Result", "violations max_lip_depth ins stats")


def check(code, lds_slots):
    """Result(violations, max_lip_depth, ins, stats) of one lowered program. stats: what the walk saw, for the tests that must
    not pass vacuously (names -> counts, "outer" gates with a context, "hxy_behind_target" flagged consumers reached with a register
    that went through a meet)."""
    code = np.asarray(code, np.uint32)
    f32 = code.view(np.float32)
    ins, bad = decode(code)
    stats = {}
    if bad:
        return Result(bad, 0, ins, stats)
    end_pc = ins[-1].pc
    at = {i.pc: k for k, i in enumerate(ins)}

    def V(i, what):
        bad.append(Violation(i.pc, i.name, what))

    tok = [0]
    ambiguous = set()

    def fresh(amb=False):
        tok[0] += 1
        if amb:
            ambiguous.add(tok[0])
        return tok[0]

    st = _State()
    st.xy, st.z, st.hxy, st.cols, st.R, st.dep, st.lip = fresh(), fresh(), None, {}, False, [1, 2, 4], ()
    pending = {}            # target pc -> [(state, origin Ins, hxy token a flagged D_SKIP promises or None)]
    dom_named = set()       # pcs of the D_LIP_PUSH instructions some D_LIP_DOM named
    skip_ids = {}
    max_depth = 0
    met_hxy = set()         # hxy tokens that were the same on every path of some meet where the paths really differed

    def drop(i, entries):
        for e in entries:
            if e not in dom_named:
                V(i, f"drops the interval-stack entry pushed at {e}, which was neither popped nor named by a D_LIP_DOM")

    def col_read(i, c, want=None):
        if c >= lds_slots:
            V(i, f"reads column {c}, at or beyond lds_slots = {lds_slots}")
            return None
        v = st.cols.get(c)
        if v is None:
            V(i, f"reads column {c}, which is not written on every path that gets here")
            return None
        if want is not None:
            if v[0] == "amb":
                V(i, f"loads a position from column {c}, whose content depends on the path taken")
                return None
            if v[0] != want:
                V(i, f"loads P.{want[1]} from column {c}, which holds {v[0]}")
                return None
            if v[1] in ambiguous:
                V(i, f"loads a position from column {c}, saved from a position that depends on the path taken")
        return v

    def col_write(i, c, v):
        if c >= lds_slots:
            V(i, f"writes column {c}, at or beyond lds_slots = {lds_slots}")
        else:
            st.cols[c] = v

    def meet(a, b):
        """b joins a (in place)."""
        if a.xy != b.xy:
            a.xy = fresh(True)
        if a.z != b.z:
            a.z = fresh(True)
        if a.hxy != b.hxy:
            a.hxy = None
        elif a.hxy is not None:
            met_hxy.add(a.hxy)
        cols = {}
        for c, v in a.cols.items():
            w = b.cols.get(c)
            if w is None:
                continue
            cols[c] = v if v == w else ("amb", fresh(True), v[2] | w[2])
        a.cols = cols
        a.R = a.R and b.R
        a.dep = [p | q for p, q in zip(a.dep, b.dep)]
        k = 0
        while k < min(len(a.lip), len(b.lip)) and a.lip[k] == b.lip[k]:
            k += 1
        dropped = a.lip[k:] + b.lip[k:]
        a.lip = a.lip[:k]
        return dropped

    def target_of(i, dist, kinds):
        """The instruction a skip of `dist` words from i lands on, or None (reported)."""
        t = i.pc + dist
        if dist <= 0:
            V(i, f"skip of {dist} words is not forward")
        elif t > end_pc:
            V(i, f"skip to {t} lands beyond D_END at {end_pc}")
        elif t not in at:
            V(i, f"skip to {t} does not land on an instruction boundary")
        elif ins[at[t]].name not in kinds:
            V(i, f"skip to {t} lands on {ins[at[t]].name}")
        else:
            return ins[at[t]]
        return None

    for k, i in enumerate(ins):
        name, pc, w, slot = i.name, i.pc, i.word, i.slot
        stats[name] = stats.get(name, 0) + 1
        # ---- paths that skipped to here
        for s, origin, promised in pending.pop(pc, ()):
            if promised is not None and st.hxy != promised:
                V(origin, "D_FLAG_HXY on D_SKIP: the subtree does not leave hypot of the entry position in the register")
            # what the target reads of the LDS (a D_LIP_DOM and the combine behind it) was written on THAT path: reported at the skip
            for t in (i, ins[k + 1]) if name == "D_LIP_DOM" else (i,):
                for c in range(t.slot, t.slot + (TABLE[t.name][2] if t.name in TABLE and t.name not in ("D_LOADP3", "D_LOADP2") else 0)):
                    if c not in s.cols:
                        V(origin, f"skip to {pc}: {t.name} reads column {c}, which the skipping path has not written")
            drop(origin, meet(st, s))
        spec = TABLE.get(name)
        if spec is None:
            V(i, "opcode without an entry in the checker's table")
            continue
        reads, writes, ncr, ncw, hxy, dep = spec
        # ---- flags
        if (w & FLAG_SHXY) and ((st.dep[0] | st.dep[1]) & 4):
            V(i, "D_FLAG_SHXY, but P.x / P.y depend on the entry z")
        if (w & FLAG_SHZ) and (st.dep[2] & 3):
            V(i, "D_FLAG_SHZ, but P.z depends on the entry x / y")
        if (w & FLAG_HXY) and hxy is None:
            V(i, "D_FLAG_HXY on an instruction that does not take it")
        if (w & FLAG_SWAP) and name not in SWAP_TAKERS:
            V(i, "D_FLAG_SWAP on an instruction that does not take it")
        # ---- reads
        if "R" in reads and not st.R:
            V(i, "reads R, which is not defined on every path that gets here")
        if hxy in ("ensure", "use") and (w & FLAG_HXY):
            if st.hxy != st.xy:
                V(i, "D_FLAG_HXY, but the register does not hold hypot of the current P.xy on every path")
            elif st.hxy in met_hxy:
                stats["hxy_behind_target"] = stats.get("hxy_behind_target", 0) + 1
        colv = []
        if name in ("D_LOADP3", "D_LOADP2"):
            colv = [col_read(i, slot + j, ("px", "py", "pz")[j]) for j in range(ncr)]
        elif name == "D_LIP_SEAM":
            if int(code[pc + 1]) & 8:
                colv = [col_read(i, slot + j) for j in range(2)]
        elif name not in ("D_LIP_PUSH", "D_LIP_POP"):
            colv = [col_read(i, slot + j) for j in range(ncr)]
        # ---- the instruction
        old_dep = list(st.dep)
        if name in GATES or name == "D_SKIP":
            taken = st.copy()
            taken.R = True
            if name == "D_SKIP":
                sid, sw = int(code[pc + 1]), int(code[pc + 3])
                if sid >= 16:
                    V(i, f"brick-mask number {sid} is not below 16")
                if sid in skip_ids:
                    V(i, f"brick-mask number {sid} is also that of the D_SKIP at {skip_ids[sid]}")
                skip_ids.setdefault(sid, pc)
                if sw >> 24:
                    V(i, "D_SKIP's skip word carries a top byte")
                promised = None
                if w & FLAG_HXY:
                    taken.hxy = promised = st.xy
                t = target_of(i, sw & 0xFFFFFF, ("D_SAVER", "D_LIP_DOM") + COMBINES)
                if t is not None:
                    pending.setdefault(t.pc, []).append((taken, i, promised))
            else:
                i0 = GATES[name]
                oslot, sw = int(code[pc + 1 + i0 + 2]), int(code[pc + 1 + i0 + 5])
                if oslot != 0xFFFF:
                    stats["outer"] = stats.get("outer", 0) + 1
                    col_read(i, oslot)
                t = target_of(i, sw & 0xFFFFFF, ("D_LIP_DOM",) + COMBINES)
                if t is not None:
                    comb = ins[at[t.pc] + 1] if t.name == "D_LIP_DOM" else t
                    if comb.name not in COMBINES or comb.slot != slot:
                        V(i, f"skip to {t.pc} lands in front of {comb.name} on slot {comb.slot}, not the combine of the gate's slot {slot}")
                    pending.setdefault(t.pc, []).append((taken, i, None))
                if sw >> 24:
                    prev = ins[k - 1] if k else None
                    if prev is None or prev.name != "D_SKIP" or int(code[prev.pc + 1]) != (sw >> 24) - 1:
                        V(i, f"the gate's brick-mask number {(sw >> 24) - 1} is not that of a D_SKIP directly in front of it")
                    elif prev.pc + (int(code[prev.pc + 3]) & 0xFFFFFF) != pc + (sw & 0xFFFFFF):
                        V(i, "the gate and the D_SKIP in front of it skip to different places")
                        V(prev, "the D_SKIP and the gate behind it skip to different places")
        elif name in ("D_LOADP3", "D_LOADP2"):
            if all(v is not None for v in colv):
                if colv[0][1] != colv[1][1]:
                    V(i, f"columns {slot} and {slot + 1} hold x and y of different positions")
                st.xy = colv[0][1]
                st.dep[0], st.dep[1] = colv[0][2], colv[1][2]
                if name == "D_LOADP3":
                    st.z, st.dep[2] = colv[2][1], colv[2][2]
            else:
                st.xy = fresh()
                if name == "D_LOADP3":
                    st.z = fresh()
        elif name in ("D_SAVEP3", "D_SAVEP2"):
            col_write(i, slot, ("px", st.xy, st.dep[0]))
            col_write(i, slot + 1, ("py", st.xy, st.dep[1]))
            if name == "D_SAVEP3":
                col_write(i, slot + 2, ("pz", st.z, st.dep[2]))
        elif name == "D_LIP_PUSH":
            if slot > len(st.lip):
                V(i, f"pushes at interval-stack level {slot}, the interval stack's depth is {len(st.lip)}")
            drop(i, st.lip[slot:])
            st.lip = st.lip[:slot] + (pc,)
            max_depth = max(max_depth, len(st.lip))
        elif name == "D_LIP_POP":
            if slot >= len(st.lip):
                V(i, f"pops interval-stack level {slot}, the interval stack's depth is {len(st.lip)}")
            else:
                if st.lip[slot] in dom_named:
                    V(i, f"pops interval-stack level {slot}, which holds a combine frame's entry (pushed at {st.lip[slot]})")
                drop(i, st.lip[slot + 1:])
                st.lip = st.lip[:slot]
        elif name == "D_LIP_DOM":
            kind, ida, idb, pinfo = int(code[pc + 1]), int(code[pc + 2]), int(code[pc + 3]), int(code[pc + 5])
            comb = ins[k + 1]
            if comb.name not in DOM_KIND or DOM_KIND[comb.name] != kind or comb.slot != slot or (comb.word ^ w) & FLAG_SWAP:
                V(i, f"is followed by {comb.name} on slot {comb.slot}: not the combine of its kind, slot and swap flag")
            for v in (ida, idb):
                if v != 0xFF and v not in skip_ids:
                    V(i, f"names brick-mask number {v}, which no D_SKIP in front of it carries")
            if (pinfo & 0xFFFF) >= len(st.lip):
                V(i, f"names interval-stack level {pinfo & 0xFFFF}, the depth is {len(st.lip)}")
            else:
                dom_named.add(st.lip[pinfo & 0xFFFF])
        else:
            # -- structure of the variable forms and the tables
            if name == "D_POLY2D":
                if ((pc + 4 + 7) & ~7) % 8 or pc + i.n > end_pc:
                    V(i, "edge records off their 8-word boundary or beyond D_END")
            elif name in ("D_LINES2D", "D_UBOUND2D", "D_UBOUND3D"):
                if pc + i.n > end_pc:
                    V(i, "the count runs beyond D_END")
            elif name == "D_CIRC_PRE":
                tab, ncirc = int(code[pc + 4]), float(f32[pc + 2])
                if tab != 0 and not (tab > end_pc and ncirc >= 0 and tab + 2 * ncirc <= len(code)):
                    V(i, f"table offset {tab} with {ncirc} entries does not lie behind D_END at {end_pc} and inside the code of {len(code)} words")
            # -- hxy
            if hxy == "ensure" and not (w & FLAG_HXY):
                st.hxy = st.xy
            # -- writes
            wr = writes
            if name == "D_TRANSLATE":
                wr = ("xy" if (f32[pc + 1] != 0 or f32[pc + 2] != 0) else "") + ("z" if f32[pc + 3] != 0 else "")
            elif name == "D_SYMMETRY":
                wr = ("xy" if int(code[pc + 1]) & 3 else "") + ("z" if int(code[pc + 1]) & 4 else "")
            if "x" in wr or "y" in wr:
                st.xy = fresh()
            if "z" in wr:
                st.z = fresh()
            if "R" in wr:
                st.R = True
            # -- dependencies
            dx, dy, dz = old_dep
            if dep == "matrix3":
                m = f32[pc + 1:pc + 13].reshape(3, 4)
                st.dep = [_mix(old_dep, m[r, :3]) for r in range(3)]     # (column 3 is the translation)
            elif dep == "matrix2":
                m = f32[pc + 1:pc + 5].reshape(2, 2)
                st.dep[:2] = [_mix(old_dep, m[r]) for r in range(2)]
            elif dep == "twist" or dep == "screw":
                st.dep[0] = st.dep[1] = dx | dy | dz
            elif dep == "revolve":
                st.dep[0] = dx | dz
            elif dep == "circ":
                st.dep[0] = st.dep[1] = dx | dy
            elif dep in ("columns3", "columns2"):
                for j in range(3 if dep == "columns3" else 2):
                    st.dep[j] = colv[j][2] if colv[j] is not None else 7
            # -- column writes
            if name == "D_CIRC_PRE":
                t0 = fresh()
                col_write(i, slot, ("px", t0, dx | dy))
                col_write(i, slot + 1, ("py", t0, dx | dy))
            elif name == "D_CIRC_ORDER":     # the two copies may change places: either is a position, which one depends on the wave
                t0 = fresh()
                cd = (colv[0][2] | colv[1][2]) if None not in colv else 7
                col_write(i, slot, ("px", t0, dx | dy | cd))
                col_write(i, slot + 1, ("py", t0, dx | dy | cd))
                st.dep[0] = st.dep[1] = dx | dy | cd
            else:
                for j in range(ncw):
                    col_write(i, slot + j, ("value", fresh(), 0))
    for t, lst in pending.items():   # (targets beyond D_END were reported where they were read)
        for _, origin, _ in lst:
            V(origin, f"skip target {t} was never reached")
    if st.lip and any(e not in dom_named for e in st.lip):
        V(ins[-1], f"the interval stack still holds unpopped entries pushed at {[e for e in st.lip if e not in dom_named]}")
    bad.sort(key=lambda v: v.pc)
    return Result(bad, max_depth, ins, stats)
