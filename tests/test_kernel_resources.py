"""No kernel of the shipped HIP library may need scratch (private segment) memory.

Why ("No scratch, anywhere"): hipcc/hiprtc of ROCm 7.2 can place a VGPR spill store at the top of a
structurizer "Flow" block, ahead of the s_andn2_saveexec that restores the lanes which skipped the `then` side of a
divergent if/else -- those lanes never execute the store and later reload a stale value (2-D fuzz tree 708: the spilled
store index of eval_kernel<2,4,4> -> 216 results written to wrong addresses). A kernel without scratch has no spill code to
misplace, so "private_segment_fixed_size == 0" is the invariant; this test reads it from the code object's metadata
notes, host-only."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_notes(elf):
    out = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], text=True)
    rows, d = [], {}
    for line in out.splitlines():
        m = re.search(r"\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\S+)", line)
        if m:
            d[m.group(1)] = m.group(2)
        if ".wavefront_size" in line:  # last key of a kernel's record
            rows.append(d)
            d = {}
    return rows


def device_code_object(lib_path, workdir):
    """Unbundle the gfx950 code object of a HIP fat binary (llvm-objdump --offloading writes next to its input)."""
    local = os.path.join(workdir, os.path.basename(lib_path))
    shutil.copy(lib_path, local)
    subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], text=True, cwd=workdir)
    objs = [os.path.join(workdir, f) for f in sorted(os.listdir(workdir)) if "amdgcn" in f and "gfx950" in f]
    assert objs, "no gfx950 code object in " + lib_path
    return objs  # one per translation unit that owns kernels (abi_eval.hip, abi_mesh.hip, abi_indexed.hip, abi_contour.hip; abi_spec.hip owns none)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="ROCm LLVM tools not installed")
def test_no_shipped_kernel_uses_scratch():
    lib = os.path.join(ROOT, "gsdf_amd", "csrc", "libgsdfhip.so")
    assert os.path.exists(lib), "build first: python __graft_entry__.py"
    with tempfile.TemporaryDirectory() as tmp:
        rows = [r for obj in device_code_object(lib, tmp) for r in kernel_notes(obj)]
    names = [r["name"] for r in rows]
    assert len(rows) >= 30 and any("leaf_eval_kernel" in n for n in names) and any("eval_kernel" in n for n in names), names
    # one leaf phase and one flat marching pass: the library ships no second form of either (flat_march_list_kernel is the pass)
    assert not [n for n in names if "leaf_kernel" in n or "leaf_brick_kernel" in n or "flat_march_kernel" in n]
    bad = [(r["name"], r["private_segment_fixed_size"], r.get("vgpr_spill_count")) for r in rows if int(r["private_segment_fixed_size"]) != 0]
    assert not bad, f"kernels with scratch (bytes, spilled VGPRs): {bad}"
    # wave64 kernels with 256-thread workgroups: the occupancy the host counts on needs <= 512 / W VGPRs, which the
    # launch bounds already enforce -- what is checked here is only that the allocator met them without spilling VGPRs
    assert all(int(r.get("vgpr_spill_count", "0")) == 0 for r in rows)
