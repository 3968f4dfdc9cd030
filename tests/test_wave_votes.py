"""Wave votes of the evaluating kernels stay on the scalar unit (host-only: reads the shipped library's gfx950 ISA).

A compare leaves its lane mask in an SGPR pair. `__all(p)` / `__any(p)` / `__ballot(p)` of a COMPOUND predicate make the compiler
move that mask through a VGPR and back before the scalar test:

    v_cndmask_b32 vN, 0, 1, mask      ; mask -> 0 / 1 per lane
    v_cmp_ne_u32  vcc, 0, vN          ; ... -> the same mask again
    s_cmp_lg_u64  vcc, exec           ; the vote

two vector instructions of the 4-cycle class per vote, for nothing (dev_math.h: wave_mask). The evaluator
writes its votes as and / or of single-compare ballots; this test counts what is left in the kernels that inline it:

  * vote round trip: `v_cndmask_b32 vN, 0, 1|-1, mask`, vN next read by `v_cmp_(ne|eq)_u32 D, 0|1, vN`, followed within four
    instructions by `s_cmp_(eq|lg)_u64 vcc, exec|0` (the `__all` form), or within eight by `s_andn2_b64 X, exec, M` and
    `s_cmp_(eq|lg)_u64 X, 0`, M being D or an s_and / s_or of it (the `wave_all_of` form)     -> must be 0;
  * mask round trip: the same pair without the scalar compare behind it (ballots for popcount / mbcnt, booleans carried over
    branches)                                                                                -> printed per kernel, not asserted.
"""
import os
import re
import subprocess
import tempfile

import pytest

from test_kernel_resources import LLVM, ROOT, device_code_object

FAMILIES = {  # family -> does a (demangled) kernel name belong to it
    "leaf_eval_kernel": lambda n: "leaf_eval_kernel" in n,
    "prune_kernel": lambda n: re.search(r"\bprune_kernel\b", n) is not None,
    "prune_spec_kernel": lambda n: "prune_spec_kernel" in n,
    "eval_kernel": lambda n: re.search(r"\beval_kernel\b", n) is not None,
    "flat_grid_kernel": lambda n: "flat_grid_kernel" in n,
}

CNDMASK = re.compile(r"^v_cndmask_b32(?:_e64|_e32)?\s+(v\d+),\s*0,\s*(?:1|-1),\s*(\S+)$")
VCMP = re.compile(r"^v_cmp_(?:ne|eq)_u32(?:_e64|_e32)?\s+(.*)$")
SCMP_VOTE = re.compile(r"^s_cmp_(?:eq|lg)_u64\s+vcc,\s*(?:exec|0)$")
VCMP_DST = re.compile(r"^(vcc|s\[\d+:\d+\])$")
SLOGIC = re.compile(r"^s_(?:and|or|andn2|orn2|xor|xnor)_b64\s+(\S+),\s*(\S+),\s*(\S+)$")
SCMP_ZERO = re.compile(r"^s_cmp_(?:eq|lg)_u64\s+(\S+),\s*0$")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def reads_or_writes(reg, text):
    """Does the instruction text name VGPR `reg` (alone or inside a range)?"""
    n = int(reg[1:])
    for m in REG.finditer(text):
        if m.group(1) is not None:
            if int(m.group(1)) == n:
                return True
        elif int(m.group(2)) <= n <= int(m.group(3)):
            return True
    return False


def kernels_of(obj):
    """{mangled kernel name: [instruction text, ...]} of one code object."""
    out = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], text=True)
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        if ins:
            cur.append(re.sub(r"\s+", " ", ins))
    return kernels


def feeds_all_of(dst, after):
    """Does the mask `dst` of a round trip's v_cmp reach `s_andn2_b64 X, exec, M` + `s_cmp_*_u64 X, 0` in the instructions `after`?"""
    if not VCMP_DST.match(dst):
        return False
    masks = {dst}
    for k, t in enumerate(after):
        m = SLOGIC.match(t)
        if not m:
            continue
        d, a, b = (x.rstrip(",") for x in m.groups())
        if t.startswith("s_andn2_b64") and a == "exec" and b in masks:
            for v in after[k + 1:k + 3]:
                z = SCMP_ZERO.match(v)
                if z and z.group(1) == d:
                    return True
        if a in masks or b in masks:
            masks.add(d)
    return False


def round_trips(ins):
    """(vote round trips, other mask round trips) of one kernel's instruction list."""
    votes = masks = 0
    for i, t in enumerate(ins):
        m = CNDMASK.match(t)
        if not m:
            continue
        reg = m.group(1)
        for j in range(i + 1, min(i + 400, len(ins))):  # the next instruction that touches vN
            u = ins[j]
            if not reads_or_writes(reg, u):
                continue
            c = VCMP.match(u)
            if c:
                ops = [o.strip() for o in c.group(1).split(",")]
                if ops[-1] == reg and ops[-2] in ("0", "1"):
                    if any(SCMP_VOTE.match(v) for v in ins[j + 1:j + 5]) or feeds_all_of(ops[0], ins[j + 1:j + 9]):
                        votes += 1
                    else:
                        masks += 1
            break
    return votes, masks


def demangle(names):
    out = subprocess.check_output(["c++filt"], input="\n".join(names), text=True)
    return dict(zip(names, out.splitlines()))


def count_library(lib):
    """{family: {demangled kernel: (votes, masks)}} over the gfx950 code objects of a HIP fat binary."""
    res = {f: {} for f in FAMILIES}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in device_code_object(lib, tmp):
            ks = kernels_of(obj)
            names = demangle(list(ks))
            for mangled, ins in ks.items():
                nm = names[mangled].split("(")[0]
                for fam, belongs in FAMILIES.items():
                    if belongs(nm):
                        res[fam][nm] = round_trips(ins)
    return res


def test_counter_recognises_the_pattern():
    vote = ["v_cmp_eq_f32_e32 vcc, 0, v1", "v_cndmask_b32_e64 v7, 0, 1, s[0:1]", "v_add_f32_e32 v2, v3, v4", "v_cmp_ne_u32_e32 vcc, 0, v7",
            "s_cmp_lg_u64 vcc, exec", "s_cbranch_scc1 L1"]
    assert round_trips(vote) == (1, 0)
    mask = ["v_cndmask_b32_e64 v7, 0, 1, s[0:1]", "v_cmp_ne_u32_e64 s[4:5], 1, v7", "s_bcnt1_i32_b64 s6, s[4:5]"]
    assert round_trips(mask) == (0, 1)
    used = ["v_cndmask_b32_e64 v7, 0, 1, s[0:1]", "v_add_u32_e32 v8, v7, v8", "v_cmp_ne_u32_e32 vcc, 0, v7", "s_cmp_lg_u64 vcc, exec"]
    assert round_trips(used) == (0, 0)  # the 0 / 1 is a value someone needs
    ranged = ["v_cndmask_b32_e64 v7, 0, 1, s[0:1]", "global_store_dwordx2 v[10:11], v[6:7], off", "v_cmp_ne_u32_e32 vcc, 0, v7", "s_cmp_eq_u64 vcc, 0"]
    assert round_trips(ranged) == (0, 0)
    all_of = ["v_cndmask_b32_e64 v15, 0, 1, s[12:13]", "v_cmp_ne_u32_e32 vcc, 0, v15", "v_cndmask_b32_e64 v15, 0, 1, s[10:11]",
              "v_cmp_ne_u32_e64 s[10:11], 0, v15", "s_and_b64 s[10:11], s[10:11], vcc", "s_andn2_b64 s[10:11], exec, s[10:11]",
              "s_cmp_lg_u64 s[10:11], 0"]
    assert round_trips(all_of) == (2, 0)  # a wave_all_of vote whose two ballots went through a VGPR
    flag = ["v_cndmask_b32_e64 v13, 0, 1, s[10:11]", "v_cmp_ne_u32_e64 s[4:5], 1, v13", "s_andn2_b64 vcc, exec, s[10:11]", "s_cbranch_vccnz 2"]
    assert round_trips(flag) == (0, 1)  # a uniform flag inverted for the far side of a branch: a mask round trip, no vote
    clean = ["v_cmp_le_f32_e32 vcc, s0, v7", "v_cmp_ge_f32_e64 s[0:1], s1, v8", "s_and_b64 s[0:1], s[0:1], vcc", "s_cmp_eq_u64 s[0:1], exec"]
    assert round_trips(clean) == (0, 0)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")
def test_no_vote_round_trips_in_the_evaluating_kernels():
    lib = os.path.join(ROOT, "gsdf_amd", "csrc", "libgsdfhip.so")
    assert os.path.exists(lib), "build first: python __graft_entry__.py"
    res = count_library(lib)
    for fam, ks in res.items():
        for nm, (v, m) in sorted(ks.items()):
            print(f"{fam}: {nm}: vote round trips {v}, other mask round trips {m}")
        print(f"{fam}: {len(ks)} kernels, vote round trips {sum(v for v, _ in ks.values())}, other mask round trips {sum(m for _, m in ks.values())}")
    empty = [fam for fam, ks in res.items() if not ks]
    assert not empty, f"no kernel found for {empty}: renamed?"
    bad = {nm: v for ks in res.values() for nm, (v, _) in ks.items() if v}
    assert not bad, f"vote round trips (v_cndmask 0/1 -> v_cmp_ne -> s_cmp vcc, exec): {bad}"
