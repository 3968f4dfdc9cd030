"""A census of the kernel launches in gsdf_amd/csrc/abi_*.hip and abi_*.cpp (no GPU): every launch whose grid is smaller than one
workgroup per 256 elements -- sized by grid_for(...), by `num_cu * ...`, or by a constant -- must stand in tests/grid_trips.py with
the case of tests/test_gpu_grid_trips.py that drives its loop through three trips, and with the workgroups per CU the source gives
it. A launch added later without such a case fails here."""
import glob
import os
import re

import pytest

import grid_trips as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdf_amd", "csrc")
KNOB = "GSDF_HIP_GRID_CUS"


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "abi_*.hip")) + glob.glob(os.path.join(CSRC, "abi_*.cpp")))
    assert len(files) >= 8, files
    return files


def _strip_comments(text):
    """Comments blanked out (offsets kept); string literals are left alone (none of the launches has a // or /* in one)."""
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def _call_args(text, open_paren):
    """The top-level arguments of the call whose '(' is at open_paren."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i].strip())
                return args
        elif c == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    raise AssertionError("unbalanced call at offset %d" % open_paren)


def _definition(text, name, before):
    """The nearest assignment `name = ...;` that ends before offset `before`: (right-hand side, its offset), or None."""
    best = None
    for m in re.finditer(r"(?<![\w.>])" + re.escape(name) + r"\s*=(?!=)\s*([^;]+);", text[:before]):
        best = (m.group(1), m.start())
    if best:   # (one declaration may define several names: this one's initialiser ends at the first comma outside brackets)
        depth = 0
        for i, c in enumerate(best[0]):
            depth += (c in "([{") - (c in ")]}")
            if c == "," and depth == 0:
                best = (best[0][:i], best[1])
                break
    return best


def _expand(text, expr, before, depth=3):
    """expr with the definitions of the identifiers it names appended (transitively, each looked up before the text that names it)."""
    out, seen, todo = [expr], set(), [(expr, before, depth)]
    while todo:
        e, pos, d = todo.pop()
        if d == 0:
            continue
        for name in set(re.findall(r"[A-Za-z_]\w*(?:\.\w+)?", e)):
            got = _definition(text, name, pos)
            if got and (name, got[1]) not in seen:
                seen.add((name, got[1]))
                out.append(got[0])
                todo.append((got[0], got[1], d - 1))
    return " ; ".join(out)


def _kernels_of(text, expr, before):
    """The __global__ functions a launch's first argument can name: literally, through an X_aot(...) picker, or through a variable."""
    full = _expand(text, expr, before, 2)
    names = set(re.findall(r"\b(\w+_kernel)\b", full))
    names |= {m + "_kernel" for m in re.findall(r"\b(\w+)_aot\b", full)}
    return names - {"launch_kernel"}


def _blocks_per_cu(text, full):
    """The workgroups per CU of a CU-capped grid: grid_for's last argument, or the factor of num_cu; a knob's default where it is
    env_int(name, default)."""
    def value(tok):
        tok = tok.strip()
        if re.fullmatch(r"\d+u?", tok):
            return int(tok.rstrip("u"))
        m = re.search(r"\b" + re.escape(tok) + r"\s*=\s*env_int\(\s*\"\w+\"\s*,\s*(\d+)\s*\)", text)
        return int(m.group(1)) if m else None
    m = re.search(r"grid_for\(", full)
    if m:
        return value(_call_args(full, m.end() - 1)[-1])
    m = re.search(r"num_cu\s*\*\s*(?:\(\w+\)\s*)?\(?\s*(\w+)(?:\s*>\s*0\s*\?\s*\w+\s*:\s*(\d+)\s*\))?", full)
    if m:
        v = value(m.group(1))
        return v if v is not None else (int(m.group(2)) if m.group(2) else None)
    return None


def census():
    """[(file, line, kernels, kind, blocks per CU or the constant grid, grid text)] of the capped launches."""
    found = []
    for path in _sources():
        text = _strip_comments(open(path).read())
        for m in re.finditer(r"\b(LAUNCH|hipLaunchKernelGGL|launch_kernel)\s*\(", text):
            line_start = text.rfind("\n", 0, m.start()) + 1
            if text[line_start:m.start()].lstrip().startswith("#define"):
                continue
            args = _call_args(text, m.end() - 1)
            if m.group(1) == "launch_kernel":   # (kernel, its per-tree build, grid, BLOCK, ...): a template's commas split the kernel
                at = args.index("BLOCK") - 1
                kern, grid = ", ".join(args[:at]), args[at]
            else:
                kern, grid = args[0], args[1]
            if kern == "KERNEL":
                continue                # (the LAUNCH macros' own bodies)
            grid = re.sub(r"^dim3\((.*)\)$", r"\1", grid)
            kernels = _kernels_of(text, kern, m.start())
            assert kernels, (os.path.basename(path), kern)
            full = _expand(text, grid, m.start())
            line = text.count("\n", 0, m.start()) + 1
            where = (os.path.basename(path), line)
            if "grid_for(" in full or "num_cu" in full:
                found.append(where + (kernels, "cu", _blocks_per_cu(text, full), grid))
            elif re.fullmatch(r"\d+u?", grid):
                found.append(where + (kernels, "const", int(grid.rstrip("u")), grid))
            elif re.search(r"\?[^;]*:\s*\d+u\b", full):
                found.append(where + (kernels, "const", int(re.search(r":\s*(\d+)u\b", full).group(1)), grid))
    return found


def test_the_census_sees_the_launches_it_is_about():
    """The parser itself: the launch forms it must resolve (a grid in a variable, in a struct field, behind a rounding, a kernel behind
    a picker) are found, and launches with one workgroup per 256 elements are not."""
    got = {}
    for f, line, kernels, kind, cap, grid in census():
        for k in kernels:
            got.setdefault(k, []).append((f, kind, cap))
    for k, want in (("eval_kernel", ("abi_eval.hip", "cu", 64)), ("image2_kernel", ("abi_eval.hip", "cu", 8)), ("view_kernel", ("abi_eval.hip", "cu", None)),
                    ("dc_origin_kernel", ("abi_mesh.hip", "cu", 32)), ("dc_edges_kernel", ("abi_mesh.hip", "cu", 8)), ("leaf_eval_kernel", ("abi_mesh.hip", "cu", 32)),
                    ("flat_march_list_kernel", ("abi_mesh.hip", "cu", 6)), ("flat_cut_scan_kernel", ("abi_mesh.hip", "cu", 16)), ("pack_records_kernel", ("abi_mesh.hip", "cu", 8)),
                    ("march_dense_kernel", ("abi_mesh.hip", "cu", 4)), ("stl_kernel", ("abi_mesh.hip", "cu", 8)), ("weld_insert_kernel", ("abi_indexed.hip", "cu", 16)),
                    ("block_scan_kernel", ("abi_indexed.hip", "const", 1)), ("cmeas_maxbits_kernel", ("abi_contour.hip", "const", 1024))):
        assert want in got.get(k, []), (k, got.get(k))
    for k in ("ray_kernel", "project_kernel", "topo_union_kernel", "cmeas_kernel", "contour_cells_kernel", "prune_resolve_kernel", "dci_rank_kernel", "math_selftest_kernel"):
        assert k not in got, (k, got[k])       # one workgroup per 256 elements: no grid-stride loop to drive
    assert len(got) >= 45, sorted(got)


def test_every_capped_launch_has_a_multi_trip_case():
    module = open(os.path.join(ROOT, "tests", "test_gpu_grid_trips.py")).read()
    cases = set(re.findall(r"^def (test_\w+)\(", module, flags=re.M))
    missing, wrong = [], []
    for f, line, kernels, kind, cap, grid in census():
        for k in sorted(kernels):
            if k in G.FIXED_ELSEWHERE and kind == "const":
                continue
            row = G.GRID_TABLE.get(k)
            if row is None:
                missing.append("%s:%d launches %s on a capped grid (%s); tests/grid_trips.py has no multi-trip case for it" % (f, line, k, grid))
                continue
            have = ("const", row.cap[1]) if isinstance(row.cap, tuple) else ("cu", row.cap)
            if kind != have[0] or (cap is not None and cap != have[1]):
                wrong.append("%s:%d launches %s with %s %s, tests/grid_trips.py says %s %s" % (f, line, k, kind, cap, have[0], have[1]))
    assert not missing, "\n".join(missing)
    assert not wrong, "\n".join(wrong)
    for k, row in G.GRID_TABLE.items():
        for c in row.cases:
            assert c in cases, "tests/grid_trips.py gives %s the case %s, which tests/test_gpu_grid_trips.py does not define" % (k, c)
    assert set(G.READING) == set(G.GRID_TABLE), sorted(set(G.READING) ^ set(G.GRID_TABLE))   # every loop was read before it ran on one CU
    launched = {k for _, _, ks, _, _, _ in census() for k in ks}
    stale = sorted((set(G.GRID_TABLE) | set(G.FIXED_ELSEWHERE)) - launched)
    assert not stale, ("in tests/grid_trips.py but not launched on a capped grid any more", stale)


def test_a_removed_entry_fails_the_census(monkeypatch):
    table = dict(G.GRID_TABLE)
    del table["weld_insert_kernel"]
    monkeypatch.setattr(G, "GRID_TABLE", table)
    with pytest.raises(AssertionError) as e:
        test_every_capped_launch_has_a_multi_trip_case()
    assert "weld_insert_kernel" in str(e.value) and "no multi-trip case" in str(e.value)


def test_the_knob_is_read_at_every_handle_creation():
    """No `static` caches it, one helper reads it, and the handles take their CU count from that helper alone."""
    reads = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path) or not path.endswith((".h", ".hip", ".cpp")):
            continue
        text = _strip_comments(open(path).read())
        for m in re.finditer(KNOB, text):
            stmt = text[max(text.rfind(";", 0, m.start()), text.rfind("{", 0, m.start())) + 1:m.start()]
            assert not re.search(r"\bstatic\b", stmt), (os.path.basename(path), stmt.strip())
            reads.append(os.path.basename(path))
        assert "multiProcessorCount" not in text or os.path.basename(path) == "abi_host.h", os.path.basename(path)
    assert reads == ["abi_host.h"], reads
    users = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "abi_*")) if p.endswith((".h", ".hip", ".cpp")) and re.search(r"\bgrid_cus\(", _strip_comments(open(p).read()))}
    assert users == {"abi_host.h", "abi_eval.hip", "abi_comm.cpp", "abi_indexed.hip"}, users
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    assert "int gsdf_hip_grid_cus(int device, int* real_cus);" in hdr
    assert KNOB in open(os.path.join(ROOT, "tools", "README.md")).read()
