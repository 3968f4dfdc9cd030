#!/usr/bin/env python3
"""bench.py -- headline benchmark: SDF evals/s + triangles/s, examples/npt-flange at resdiv 1600,
octree pruning + marching cubes on device (BASELINE.json configs[1]).

A "step" is one complete mesh of the model: every octree level, every leaf corner evaluation and all
marching-cubes triangle emission, starting from the flattened tree resident in HBM and ending with
the triangle buffer resident in HBM (N>1: + the RCCL gather of all ranks' triangles on every rank).
Positions are generated on device from the lattice, so there is no host input to upload.

  python bench.py --gpus N --steps K --warmup W            (N>1: launched by torch.distributed.run)

Prints ONE JSON line (rank 0). value = total SDF evaluations of all ranks / max-over-ranks time.

A plain run sets up, warms up, times the K steps and prints the line. --full adds every measurement beside the headline,
each after the timed loop: the roofline objects (blocking meshes with the device to itself, the live copy-kernel yardstick),
the distinct-rows / distinct-points meshes, the other gather modes (N > 1), the host-inclusive, drop-in and one-shot
timings and the CPU baseline. --dump-outputs DIR writes what the timed loop's last step computed to DIR/<name>.npy
(dump_outputs below).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
DUMP_BYTES = 48 << 20  # what --dump-outputs writes at most (under the 64 MB a dump may take)


def triangle_sample(tris, budget=DUMP_BYTES):
    """A fixed sample of a triangle set that does not depend on the order the device emitted it in: the triangles whose 32-bit
    hash of their nine coordinates' bits falls in one of 2^k buckets (k the smallest that fits `budget`), sorted bitwise.
    Two builds that make the same triangle set give the same array; one triangle more or less changes one row. (m, 9) float32."""
    import numpy as np
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    k = 0
    while (t.shape[0] * 36) >> k > budget:
        k += 1
    if k:
        u = t.view(np.uint32)
        h = np.full(t.shape[0], 2166136261, np.uint32)  # FNV-1a over the nine words, then a final mix
        for c in range(9):
            h ^= u[:, c]
            h *= np.uint32(16777619)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(12)
        t = t[(h & np.uint32((1 << k) - 1)) == 0]
    t = t[np.lexsort(t.view(np.uint32).T[::-1])]
    return t[:budget // 36]


def dump_outputs(d, arrays):
    """--dump-outputs: every array as d/<name>.npy (float32 / float64)."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(d, name + ".npy"), a)


def mesh_outputs(mesh, evals):
    """What a caller of a mesh receives: its triangles (triangle_sample of them) and counts = [triangles, evaluations]."""
    import numpy as np
    if hasattr(mesh, "RenderAll"):
        tris = mesh.RenderAll()
    else:  # the torch.distributed gather's result: a device tensor of triangles
        tris = mesh.detach().cpu().numpy()
    tris = tris.reshape(-1, 9)
    return {"triangles": triangle_sample(tris), "counts": np.array([tris.shape[0], evals], np.float64)}


def cpu_baseline(shader, scene, resdiv, threads):
    """Reference CPU path for this workload (gsdfaux.RenderShader3D without -gpu: FlatRenderer over the
    batch-recursive evaluators, batch 4096, GOMAXPROCS-1 goroutines), restated in oracle/ (kind=port).
    Beside the many-thread sample of the bench workload: the same path on ONE thread, and the reference's own published
    case (README.md:125-134: npt-flange resdiv 400, 6.7 M evaluations in 313 ms = 21.4 M evals/s on 11 threads of an
    i5-12400F) at the host's thread count and at 11 threads as a sanity anchor -- SURVEY.md section 8(d)."""
    import numpy as np
    from oracle.oracle import OracleSDF

    def run(rd, nt, reps=1):
        res = np.float32(float(shader.Diagonal()) / rd)
        best = None
        for _ in range(reps):  # the small samples take the better of two: the first pass pays page faults and thread start-up
            sdf = OracleSDF(shader.tree())
            t0 = time.perf_counter()
            m = sdf.render_flat(res, 4096, nt)
            dt = time.perf_counter() - t0
            if best is None or dt < best[1]:
                best = (m, dt)
        return best

    m, dt = run(resdiv, threads)
    out = {"value": m.evals / dt, "unit": "evals/s", "cores": threads, "kind": "port",
           "sample": f"{scene} resdiv {resdiv} flat lattice {m.grid[0]+1}x{m.grid[1]+1}x{m.grid[2]+1} = {m.evals} evals, "
                     f"{m.n_tris} triangles in {dt:.2f}s (FlatRenderer+batch-recursive evaluators, batch 4096; the FLAT lattice forms a corner "
                     f"as O+res*i, the octree as (O+res*(i-1))+res -- an ulp apart on some planes, hence 6818304 flat vs 6818282 octree triangles at resdiv 1600: DESIGN.md section 6)",
           "triangles_per_s": m.n_tris / dt, "eval_only_evals_per_s": m.evals / m.t_eval_s}
    m1, dt1 = run(400, 1, 2)
    out["single_thread"] = {"value": m1.evals / dt1, "unit": "evals/s", "cores": 1, "triangles_per_s": m1.n_tris / dt1,
                            "sample": f"{scene} resdiv 400: {m1.evals} evals, {m1.n_tris} triangles in {dt1:.2f}s"}
    anchor = []
    for nt in sorted({min(11, threads), threads}):
        ma, dta = run(400, nt, 2)
        anchor.append({"value": ma.evals / dta, "unit": "evals/s", "cores": nt, "triangles": ma.n_tris, "triangles_per_s": ma.n_tris / dta,
                       "seconds": dta})
    # like for like with the device's octree path: the oracle's octree renderer (same algorithm: centre tests at every level,
    # 8 corners per leaf) on one thread at resdiv 400 -- the flat lattice above evaluates 0.7x as many points at that size
    so = OracleSDF(shader.tree())
    r400 = np.float32(float(shader.Diagonal()) / 400)
    t0 = time.perf_counter()
    mo = so.render_octree(r400, 4096, True)
    dto = time.perf_counter() - t0
    out["octree_single_thread"] = {"value": mo.evals / dto, "unit": "evals/s", "cores": 1, "triangles_per_s": mo.n_tris / dto,
                                   "sample": f"{scene} resdiv 400 octree renderer: {mo.evals} evals, {mo.n_tris} triangles in {dto:.2f}s"}
    out["resdiv400"] = {"runs": anchor, "reference_published": {"value": 6711686 / 0.313, "unit": "evals/s", "cores": 11,
                                                                "hardware": "i5-12400F (README.md:125-134)", "triangles": 423852}}
    return out


def host_inclusive(hip, sdf, res, reps=7):
    """What the reference's caller ends up with (gsdfaux.RenderShader3D: triangles in host memory, glrender/glrender.go:17-36,
    then an STL file, stl.go:15-62), timed AFTER the contract's timed loop so that it does not perturb it: one mesh + its
    triangles by one DMA into pinned host memory (gsdf_hip_mesh_host_tris), and one mesh + the complete binary STL file built
    on device and moved the same way (gsdf_hip_mesh_host_stl). PCIe-inclusive: never the headline value. Median of `reps`."""
    import statistics
    out = {}
    for key, view in (("ms_tris_host", "triangles_view"), ("ms_stl_host", "stl_view")):
        ts, nbytes = [], 0
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            oc = hip.OctreeHIP(sdf, res)
            v = getattr(oc, view)()
            ts.append((time.perf_counter() - t0) * 1e3)
            nbytes = int(v.nbytes)
            del v, oc
        out[key] = statistics.median(ts[1:])  # (the first pass pins the host buffer)
        out[key.replace("ms_", "bytes_")] = nbytes
    out["note"] = ("one complete mesh + result in host memory per call (pinned buffer from the library's pool, one DMA); "
                   "the headline stops at triangles resident in HBM")
    return out


def one_shot(hip, shader, res):
    """What every example of the reference does once (examples/npt-flange/flange.go:61-98; README.md:109-120: GL init 53.5 ms +
    shader compile 7.7 ms + render 706 ms + STL 371 ms at resdiv 400): tree -> binary STL bytes in host memory, from a COLD
    handle, wall clock, timed AFTER the contract's timed loop (the process, its HIP context and the library's ahead-of-time
    kernels are warm; the handle, its device workspaces, its specialised kernels are not). Five ways to get there:
      interpreter        create, mesh through the ahead-of-time interpreter kernels, STL
      specialise_cold    create, gsdf_hip_program_specialize with an EMPTY code-object cache (the installed hipcc, out of process), mesh, STL
      cache_hit          the same with the cache filled by the previous row (GSDF_HIP_CACHE_DIR): the build is a file read
      async_cold         create, gsdf_hip_program_specialize_async with an empty cache, mesh AT ONCE (interpreter kernels: the build is still running), STL
      async_warm         the same with the cache warm (the mesh takes whichever kernels are ready when it is enqueued)
    The policy for a one-mesh caller is the last two: never wait for a compiler. PCIe-inclusive, never the headline value."""
    import shutil
    import statistics
    import tempfile

    def run(prepare):
        t0 = time.perf_counter()
        sdf = hip.SDF3HIP(shader)
        t1 = time.perf_counter()
        prepare(sdf)
        t2 = time.perf_counter()
        oc = hip.OctreeHIP(sdf, res)
        t3 = time.perf_counter()
        v = oc.stl_view()
        nbytes = int(v.nbytes)
        t4 = time.perf_counter()
        leaf = sdf.info()["kernels"].get("leaf")
        ntris = int(oc.n_tris())
        del v, oc
        sdf.close()  # (waits for a background build still under way: outside the timed span)
        return {"ms": (t4 - t0) * 1e3, "ms_create": (t1 - t0) * 1e3, "ms_prepare": (t2 - t1) * 1e3, "ms_mesh": (t3 - t2) * 1e3,
                "ms_stl_to_host": (t4 - t3) * 1e3, "stl_bytes": nbytes, "triangles": ntris, "leaf_kernel_at_the_end": leaf}

    def med(rows):
        r = dict(rows[len(rows) // 2])
        for k in ("ms", "ms_create", "ms_prepare", "ms_mesh", "ms_stl_to_host"):
            r[k] = statistics.median(x[k] for x in rows)
        return r

    old = os.environ.get("GSDF_HIP_CACHE_DIR")
    d1, d2 = tempfile.mkdtemp(prefix="gsdf_oneshot_"), tempfile.mkdtemp(prefix="gsdf_oneshot_")
    out = {}
    try:
        os.environ["GSDF_HIP_CACHE_DIR"] = d1
        out["interpreter"] = med([run(lambda s: None) for _ in range(3)])
        out["specialise_cold"] = run(lambda s: s.specialize())
        out["cache_hit"] = med([run(lambda s: s.specialize()) for _ in range(3)])
        out["async_warm"] = med([run(lambda s: s.specialize_async()) for _ in range(3)])
        os.environ["GSDF_HIP_CACHE_DIR"] = d2
        out["async_cold"] = run(lambda s: s.specialize_async())
    finally:
        if old is None:
            os.environ.pop("GSDF_HIP_CACHE_DIR", None)
        else:
            os.environ["GSDF_HIP_CACHE_DIR"] = old
        shutil.rmtree(d1, ignore_errors=True)
        shutil.rmtree(d2, ignore_errors=True)
    out["ms"] = min(out["async_warm"]["ms"], out["cache_hit"]["ms"])
    out["note"] = ("tree -> complete binary STL file in host memory from a cold handle (wall clock, PCIe-inclusive; medians of 3 except the two rows that "
                   "run the compiler); `ms` = the better of the two warm-cache rows; the first mesh of a handle sizes its triangle buffer from a guess and "
                   "repeats the chain once with the exact size when the guess is short (ms_mesh includes it)")
    return out


def guarded(fn, *a):
    """A measurement that follows the timed loop must never cost the headline its line: its failure is reported in its place."""
    try:
        return fn(*a)
    except Exception as ex:  # noqa: BLE001
        return {"error": f"{fn.__name__}: {ex!r}"[:400]}


def evaluate_dropin(hip, sdf, shader, n=32768, calls=300):
    """The literal drop-in seam, measured AFTER the contract's timed loop: gleval.SDF3.Evaluate as the reference's own renderers
    call it -- one blocking call per <= 32 768 host points (gsdfaux/gsdfaux.go:108-113,170; glrender/octreerenderer.go:154-176;
    upload / dispatch / readback per call in the reference, gleval/gpu_cgo.go:194-258) -- through gsdf_hip_eval3 from pageable
    host buffers, then the same from registered (pinned, device-mapped) buffers and as pipelined submit / wait pairs. Points:
    the npt-flange lattice at resdiv 400 (the reference's published case), 32 768 per call. PCIe- and launch-latency-bound by
    construction: never the headline value. The loop is Python over raw ctypes calls (~2 us of the per-call figure)."""
    import ctypes as C
    import numpy as np
    L = hip.lib()
    bb = shader.Bounds().astype(np.float64)
    res = float(shader.Diagonal()) / 400
    rng = np.random.default_rng(5)
    base = (bb[:3] + rng.random((n, 3)) * (bb[3:] - bb[:3])).astype(np.float32)
    base = (np.floor(base / res) * res).astype(np.float32)  # lattice-like coordinates (exact multiples share x, y, z values as a renderer's batches do)
    out = {"points_per_call": n, "calls": calls, "unit": "evals/s"}

    def run(label, bufs, pipelined):
        h = sdf._h
        ptrs = [(p_.ctypes.data, d_.ctypes.data) for p_, d_ in bufs]
        tick = [C.c_int(), C.c_int()]
        rc = 0
        for rep in range(2):  # the first pass warms the slots' staging buffers
            t0 = time.perf_counter()
            if not pipelined:
                pp, dp = ptrs[0]
                for _ in range(calls):
                    rc |= L.gsdf_hip_eval3(h, pp, 12, n, dp, n)
            else:  # two calls in flight: submit the next batch, then wait for the previous one
                live = [False, False]
                for k in range(calls):
                    i = k & 1
                    if live[i]:
                        rc |= L.gsdf_hip_eval_wait(h, tick[i])
                    rc |= L.gsdf_hip_eval3_submit(h, ptrs[i][0], 12, n, ptrs[i][1], n, C.byref(tick[i]))
                    live[i] = True
                for i in range(2):
                    if live[i]:
                        rc |= L.gsdf_hip_eval_wait(h, tick[i])
            dt = time.perf_counter() - t0
        assert rc == 0, L.gsdf_hip_last_error()
        out[label] = {"evals_per_s": n * calls / dt, "us_per_call": dt / calls * 1e6}

    page = [(base.copy(), np.empty(n, np.float32)) for _ in range(2)]
    reg = [(hip.host_array((n, 3)), hip.host_array((n,))) for _ in range(2)]
    for p_, _ in reg:
        p_[:] = base
    run("blocking_pageable", page, False)
    run("blocking_registered", reg, False)
    assert (page[0][1].view(np.uint32) == np.asarray(reg[0][1]).view(np.uint32)).all()
    run("pipelined_pageable", page, True)
    run("pipelined_registered", reg, True)
    assert (page[1][1].view(np.uint32) == np.asarray(reg[1][1]).view(np.uint32)).all() and (page[1][1].view(np.uint32) == page[0][1].view(np.uint32)).all()
    out["note"] = ("gleval.SDF3.Evaluate through gsdf_hip_eval3, one call per 32768 host points as the reference's renderers issue them; "
                   "PCIe- and launch-latency-inclusive, never the headline")
    return out


VALU_PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9  # MI355X_MICROARCH.md: 256 CUs x 4 SIMD-32, one wave64 VALU op per 2 cycles, 2.4 GHz


def _pmc_files(workload, want):
    """Committed rocprofv3 PMC summaries (profiles/*_pmc_summary.json) of THIS workload (scene and resdiv), newest first; `want(j)` picks
    the kind (octree / dual contouring)."""
    import glob
    import re
    key = re.match(r"examples/(\S+) resdiv (\d+)", workload or "")
    if not key:
        return
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")), reverse=True):
        try:
            j = json.load(open(f))
        except Exception:
            continue
        k2 = re.match(r"examples/(\S+) resdiv (\d+)", j.get("workload", ""))
        if k2 and k2.groups() == key.groups() and want(j):
            yield f, j


def pmc_summary(workload, code=None):
    """Counters of the evaluating kernel for THIS workload from the committed profiles: the newest summary whose code key
    (gsdf_hip_program_kernels: a hash of the kernels' sources and the program) equals the running kernels' -> code_match True;
    failing that the newest one of the workload with code_match False (the line says so: roofline.counters). A line never carries
    another workload's counters. {} if there is none."""
    first = None
    for f, j in _pmc_files(workload, lambda j: j.get("leaf_eval_kernel") or j.get("leaf_kernel")):
        d = dict(j.get("leaf_eval_kernel") or j.get("leaf_kernel"), source=os.path.basename(f))
        if code is None or j.get("code") == code:
            return dict(d, code_match=True)
        first = first or dict(d, code_match=False)
    return first or {}


def pmc_dc_stages(workload, code=None):
    """Per-stage counters of the dual contouring kernels, chosen like pmc_summary: ({stage: {...}}, code_match)."""
    first = None
    for f, j in _pmc_files(workload, lambda j: "dc_origin_kernel" in j and "dual contouring" in j.get("workload", "")):
        out = {}
        for st in ("dc_block_test", "dc_origin", "dc_edges", "dc_normals", "dc_place", "dc_quads"):
            d = j.get(st + "_kernel")
            if d:
                out[st] = {k: d[k] for k in ("SQ_INSTS_VALU", "SQ_INSTS_LDS", "hbm_traffic_gb_per_launch", "wave_wait_any_frac", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE") if k in d}
                out[st]["counters_from"] = os.path.basename(f)
        if code is None or j.get("code") == code:
            return out, True
        first = first or (out, False)
    return first or ({}, None)


def counters_note(source, match):
    """Where a line's instruction / traffic counters come from -- never measured by bench.py itself (PMC needs rocprofv3)."""
    if not source:
        return "none: no committed PMC summary of this workload (achieved / frac / traffic are null)"
    return (f"read from profiles/{source} (rocprofv3 --pmc passes of this workload, tools/gpu_profile.sh), not measured in this run; "
            + ("its code key equals the running kernels'" if match else "its code key DIFFERS from the running kernels': the kernels were edited after that profile"))


def copy_rate_gbs(rbytes, wbytes):
    """Live: GB/s a plain HIP copy kernel (16 B per lane, best of plain / nontemporal variants and grid sizes) reaches on this box
    for a stream of `rbytes` read + `wbytes` written (tools/ubench/copy_rate.hip, built by __graft_entry__.build()). None if unbuilt."""
    import ctypes as C
    so = os.path.join(ROOT, "tools", "ubench", "libcopyrate.so")
    if not os.path.exists(so):
        return None
    L = C.CDLL(so)
    L.copy_rate_ms.restype = C.c_float
    L.copy_rate_ms.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]
    best = None
    for v, name in ((0, "plain"), (1, "nt-store"), (2, "nt-load+store")):
        for bpc in (4, 8, 16):
            ms = L.copy_rate_ms(int(rbytes), int(wbytes), v, 30, bpc)
            if ms > 0 and (best is None or ms < best[0]):
                best = (ms, name, bpc)
    if best is None:
        return None
    return {"gb_per_s": (rbytes + wbytes) / (best[0] * 1e-3) / 1e9, "ms": best[0], "variant": best[1], "workgroups_per_cu": best[2]}


def valu_roofline(kernel_evals_per_s, workload, code=None):
    """The binding roofline of this path: VALU issue. Instructions per evaluation come from the PMC pass of the same
    workload (SQ_INSTS_VALU x 64 lanes / evaluations per launch), the rate from the live kernel timing."""
    pm = pmc_summary(workload, code)
    per_eval = pm.get("valu_lane_instr_per_eval")
    if not per_eval:
        return None
    ach = per_eval * kernel_evals_per_s
    out = {"lane_instr_per_eval": per_eval, "counters_from": pm.get("source"), "code_match": pm.get("code_match"), "achieved": ach / 1e12, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "T lane-instr/s",
           "frac": ach / VALU_PEAK_LANE_OPS}
    mix = pm.get("valu_mix")
    if mix and mix.get("cycles_per_instr_by_class"):
        # what the kernel's own instruction mix allows: classes priced by their measured issue cost in real shader cycles, at the
        # clock VALU-dense code runs at (tools/ubench/class_rate.hip; the peak assumes 2 cycles for every instruction at 2.4 GHz)
        roof = 256 * 4 * 64 * mix.get("clock_ghz", 2.4) * 1e9 / mix["cycles_per_instr_by_class"]  # lanes x (clock under load) / (cycles per wave-instruction of the mix)
        out["mix"] = {k: v for k, v in mix.items() if k not in ("kernel_ms", "frac_of_mix_roof", "roof_ms")}
        out["mix_roof"] = roof / 1e12
        out["mix_roof_frac"] = ach / roof
    return out


def eval_mode(args, torch, np, hip, shader, sdf, res, dev):
    """M1: dist[i] = SDF(pos[i]) over the FlatRenderer lattice (flatrenderer.go:153-160 order), positions and distances
    resident in HBM, 2^24 points per launch. Algorithmic traffic 16 B/eval (12 B position + 4 B distance)."""
    bb = shader.Bounds().astype(np.float64)
    c, h = (bb[:3] + bb[3:]) / 2, (bb[3:] - bb[:3]) / 2 * 1.01
    mn = (c - h).astype(np.float32)
    nx, ny, nz = [int(np.ceil(np.float32(2 * h[a]) / res)) + 1 for a in range(3)]
    n = 1 << (26 if args.scene == "sphere" else 24)
    total = nx * ny * nz
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    pos = torch.empty((n, 3), device=dev, dtype=torch.float32)
    dist = torch.empty(n, device=dev, dtype=torch.float32)

    def fill(chunk):
        g = (idx + chunk * n) % total
        pos[:, 0] = mn[0] + (g % nx).to(torch.float32) * float(res)
        pos[:, 1] = mn[1] + ((g // nx) % ny).to(torch.float32) * float(res)
        pos[:, 2] = mn[2] + (g // (nx * ny)).to(torch.float32) * float(res)
    fill(0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = torch.cuda.Stream(device=dev)  # a real (non-null) stream: kernels and events must share it
    torch.cuda.synchronize()
    with torch.cuda.stream(ts):
        for _ in range(args.warmup):
            sdf.evaluate_dev(pos.data_ptr(), 12, dist.data_ptr(), n, ts.cuda_stream)
        ts.synchronize()
        t0 = time.perf_counter()
        ev0.record(ts)
        for k in range(args.steps):
            sdf.evaluate_dev(pos.data_ptr(), 12, dist.data_ptr(), n, ts.cuda_stream)
        ev1.record(ts)
        ts.synchronize()
    dt = time.perf_counter() - t0
    k_ms = ev0.elapsed_time(ev1) / args.steps
    achieved = n * 16.0 / (k_ms * 1e-3) / 1e9
    if args.dump_outputs:  # the distances of the last launch, every step-th one if all of them exceed the budget
        stride = -(-n * 4 // DUMP_BYTES)
        dump_outputs(args.dump_outputs, {"distances": dist[::stride].cpu().numpy()})
    print(json.dumps({
        "metric": "sdf_evals_per_s", "value": n * args.steps / dt, "unit": "evals/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"Evaluate micro-benchmark: {args.scene}, {n} HBM-resident lattice points per launch (lattice {nx}x{ny}x{nz} at resdiv {args.resdiv})"},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": None, "kernel": "eval_kernel<3,K>", "kernel_ms": k_ms}}), flush=True)


def flat_mode(args, torch, np, hip, shader, sdf, res, spec_note):
    """glrender.FlatRenderer on device (gsdf_hip_mesh_flat): every corner of the lattice, then marching cubes of every
    cube. Two phases with different roofs: the lattice pass is VALU-bound like the octree's leaf kernel; the marching
    pass is priced, as SURVEY 8(d) counts it, at 4 B per corner + 36 B per triangle. Since round 2 it no longer streams the
    float grid: the lattice pass leaves two bits per corner, flat_cut_scan_kernel reads those (1/16 of the bytes) and
    flat_march_list_kernel fetches the eight distances of the cut cubes only -- the figure is notional like the octree's
    (GSDF_HIP_FLAT_STREAM=1 brings back flat_march_kernel, which streams)."""
    streaming = os.environ.get("GSDF_HIP_FLAT_STREAM", "0") not in ("", "0")
    for _ in range(args.warmup):
        hip.FlatHIP(sdf, res)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g_ms = m_ms = 0.0
    for _ in range(args.steps):
        f = hip.FlatHIP(sdf, res)
        g_ms += f.stats.ms_leaf
        m_ms += f.stats.ms_march
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ev, nt = int(f.stats.evals), int(f.stats.n_tris)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, mesh_outputs(f, ev))
    g_ms /= args.steps
    m_ms /= args.steps
    alg_gb = (4.0 * ev + 36.0 * nt) / 1e9
    # dominant kernel: the lattice pass (flat_grid_kernel, 80 % of a mesh), VALU-bound like the octree's leaf kernel; its instruction
    # count from the newest committed PMC summary of the flat renderer (tools/gpu_profile.sh ... --mode flat), if any
    import glob
    vi = src = match = None
    code = sdf.info()["kernels"].get("code")
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_flat_pmc_summary.json")), reverse=True):
        j = json.load(open(f))
        if args.scene in j.get("workload", "") and str(args.resdiv) in j.get("workload", "") and "flat_grid_kernel" in j and (vi is None or j.get("code") == code):
            vi, src, match = j["flat_grid_kernel"].get("SQ_INSTS_VALU"), os.path.basename(f), (j.get("code") == code)  # the newest, or the one of this code
            traffic = j["flat_grid_kernel"].get("hbm_traffic_gb_per_launch")
            if match:
                break
    ach = vi * 64 / (g_ms * 1e-3) if vi else None
    print(json.dumps({
        "schema": 6,
        "metric": "sdf_evals_per_s", "value": ev * args.steps / dt, "unit": "evals/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"FlatRenderer on device: {args.scene} resdiv {args.resdiv}, {ev} lattice corners, {nt} triangles; {spec_note}", "code": code},
        "triangles": nt, "triangles_per_s": nt * args.steps / dt,
        "roofline": {"bound": "valu", "kernel": "flat_grid_kernel<K>", "kernel_ms": g_ms, "kernel_evals_per_s": ev / (g_ms * 1e-3),
                     "achieved": ach / 1e12 if ach else None, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "T lane-instr/s", "frac": ach / VALU_PEAK_LANE_OPS if ach else None,
                     "traffic": traffic if vi else None, "traffic_unit": "GB per launch (PMC: 2*FETCH_SIZE + WRITE_SIZE)", "counters": counters_note(src, match),
                     "hbm_notional": {"algorithmic_gb_per_launch": 16.0 * ev / 1e9, "gb_per_s": 16.0 * ev / 1e9 / (g_ms * 1e-3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "note": "16 B per lattice corner as SURVEY 8(d) counts an evaluation; the kernel writes the 4-B distance and two sign bits, positions are generated in registers"}},
        "roofline_march": {"bound": "hbm", "kernel": "flat_march_kernel" if streaming else "flat_cut_scan_kernel + flat_march_list_kernel",
                           "kernel_ms": m_ms, "algorithmic_gb_per_launch": alg_gb, "notional_gb_per_s": alg_gb / (m_ms * 1e-3),
                           "note": "marching phase (both kernels) priced as SURVEY 8(d) counts it, 4 B per corner + 36 B per triangle -- NOTIONAL: the bit-plane pass reads two bits per "
                                   "corner and the eight distances of the cut cubes only (measured HBM traffic: profiles/*_flat_pmc_summary.json), so no fraction of the peak is formed"}}), flush=True)


def self_launch(n):
    """Re-execute this command line as N ranks: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port <a free one> bench.py <the same arguments>. The launched form keeps working as before (WORLD_SIZE set)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL and hipIpcGetMemHandle need on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench: --gpus %d without a launcher: starting %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (default K: a step is a third of a millisecond and up to three are in flight -- with K = 10 the pipeline's fill and drain were 7 % of
    # the timed region, 0.345-0.350 ms per step against 0.323-0.327 from K = 200 on; HISTORY.md round 6, item 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resdiv", type=int, default=1600)
    ap.add_argument("--scene", default="npt-flange")
    ap.add_argument("--cpu-resdiv", type=int, default=0, help="resdiv of the bounded CPU sample (0 = pick ~10-30 s of CPU work from the core count)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-batch-throughput", action="store_true", help="(accepted, ignored: the timed loop itself keeps two meshes in flight since round 4)")
    ap.add_argument("--mode", choices=["mesh", "eval", "flat"], default="mesh",
                    help="mesh (default, BASELINE configs[1]) or eval: the gleval.SDF3.Evaluate micro-benchmark (SURVEY 8(d) M1) on "
                         "HBM-resident positions: 2^24-point chunks of the flat lattice of the scene at --resdiv; flat: the reference's other "
                         "renderer (FlatRenderer) on device, one GPU")
    ap.add_argument("--renderer", choices=["octree", "dualcontour"], default="octree",
                    help="mesh mode: octree + marching cubes (default, the headline) or dual contouring (BASELINE configs[4]; "
                         "e.g. --scene glyph-plate --resdiv 800 --renderer dualcontour)")
    ap.add_argument("--preheat", type=int, default=50, help="untimed meshes run during setup, before the W warmup steps, so that the GPU clocks are up")
    ap.add_argument("--interpreter", action="store_true", help="run the generic interpreter kernels instead of kernels specialised for the tree")
    ap.add_argument("--gather", choices=["all", "root", "none"], default="all",
                    help="N > 1: who ends up with the triangles -- all: RCCL all-gatherv, every rank gets everything (default, what "
                         "BASELINE.json names); root: rank 0 only (ncclSend/ncclRecv); none: every rank keeps its shard (counts only)")
    ap.add_argument("--payload", choices=["records", "triangles"], default="records",
                    help="N > 1, gather all / root, octree renderer: what a rank puts on the wire -- records: its packed cut-leaf records "
                         "(40 B per cut leaf = 20 B per triangle; the receiving ranks run marching cubes over everybody's records, default) "
                         "or triangles (36 B each, marched where they were made)")
    ap.add_argument("--no-one-shot", action="store_true", help="skip the cold-handle tree -> STL measurement that follows the timed loop (it runs the compiler twice)")
    ap.add_argument("--no-evaluate-dropin", action="store_true", help="skip the 32768-point host-buffer Evaluate measurement that follows the timed loop")
    ap.add_argument("--no-mesh-pipeline", action="store_true",
                    help="N = 1: one blocking gsdf_hip_mesh_octree call per step (default: gsdf_hip_mesh_octree_start / _wait, the next mesh's "
                         "chain of kernels is enqueued before the previous mesh is waited for; every one of the K meshes is started and "
                         "finished inside the timed region)")
    ap.add_argument("--mesh-depth", type=int, default=3, choices=[1, 2, 3],
                    help="N = 1, pipelined: meshes in flight on the handle (it has three workspaces and streams; 3 measured best: tools/gpu_pipe_depth.py)")
    ap.add_argument("--dc-handles", type=int, default=2, choices=[1, 2, 3, 4],
                    help="N = 1, --renderer dualcontour: handles of the tree, each with one blocking mesh in flight on a host thread of its own")
    ap.add_argument("--no-gather-pipeline", action="store_true",
                    help="N > 1: wait for a mesh's gather before meshing the next (default: the payload of mesh i moves while mesh i+1 is made)")
    ap.add_argument("--no-distinct-rows", action="store_true", help="skip the share_corners = 2 measurement that follows the timed loop (profiles of the headline's kernels alone)")
    ap.add_argument("--share-corners", type=int, nargs="?", const=1, default=0, choices=[0, 1, 2, 3],
                    help="0: every corner of every leaf, as the reference (headline); 1: each bitwise-distinct lattice corner of a brick once (older fused kernel); "
                         "2: the bitwise-distinct z rows of a brick once each (same kernels, same triangles, a quarter fewer evaluations)")
    ap.add_argument("--no-gather-modes", action="store_true",
                    help="N > 1, --full: skip the two extra timed loops (the gather modes other than --gather) that follow the headline loop")
    ap.add_argument("--full", action="store_true",
                    help="after the timed loop, also run every measurement beside the headline: roofline objects (blocking meshes, copy-kernel "
                         "yardstick), distinct rows / points, the other gather modes, host-inclusive, drop-in and one-shot timings, CPU baseline "
                         "(the --no-* options above skip single ones of them)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy: mesh modes triangles.npy (a fixed, "
                         "order-independent sample of at most 48 MB, sorted) and counts.npy ([triangles, evaluations]); eval mode distances.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as the driver starts the N = 1 line: become the launcher -- one rank per GPU under
        # torch.distributed.run on this node -- and pass the ranks' output through (rank 0 prints the one JSON line)
        raise SystemExit(self_launch(args.gpus))

    import numpy as np
    import torch
    from scaffold.builder import Builder
    from gsdf_amd import hip

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}, or without a launcher")
    dist = None
    comm = None
    torch_gather = False
    # one rank per GPU; on a box with fewer GPUs than ranks (GSDF_HIP_COMM=ipc: the library's inter-process transport for ranks that
    # share a device -- RCCL refuses those) the ranks go round the devices there are: the whole N > 1 path on one GPU, no scaling claim
    ndev = max(1, torch.cuda.device_count())
    shared_device = world > ndev
    if shared_device and os.environ.get("GSDF_HIP_COMM") != "ipc":
        raise SystemExit(f"{world} ranks on {ndev} GPU(s): set GSDF_HIP_COMM=ipc (ranks sharing a device cannot use RCCL)")
    dev_index = (local_rank % ndev) if world > 1 else 0
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    hip.init(dev.index)
    # (developer knobs, used by tools/gpu_dist1.sh to run the N > 1 code path on the one GPU a gpurun box has:
    # GSDF_BENCH_FORCE_DIST=1 takes it at world size 1, GSDF_BENCH_FORCE_TORCH_GATHER=1 also forces its fallback)
    force_dist = bool(os.environ.get("GSDF_BENCH_FORCE_DIST"))
    if world > 1 or force_dist:
        # Data plane: the library's own RCCL communicator (gsdf_hip_comm_*, one rank per GPU over xGMI) -- the triangle
        # all-gatherv runs inside libgsdfhip.so, exactly what a Go caller of the C ABI would use. Control plane
        # (rendezvous of the 128-byte RCCL id, barriers, three scalars at the end): torch.distributed over gloo.
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        try:
            ids = [hip.CommHIP.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            comm = hip.CommHIP(ids[0], rank, world)
            ok = 0 if os.environ.get("GSDF_BENCH_FORCE_TORCH_GATHER") else 1
        except Exception as e:  # librccl missing / refused: every rank must take the same path
            print("bench: library RCCL communicator unavailable on rank %d: %s" % (rank, str(e)[:300]), file=sys.stderr)
            comm, ok = None, 0
        flag = torch.tensor([ok], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag[0]) == 0:
            # fallback: the torch.distributed gather of gsdf_amd/gather.py on torch's own RCCL process group
            if comm is not None:
                comm.close()
                comm = None
            dist.destroy_process_group()
            dist.init_process_group("nccl", device_id=dev)
            torch_gather = True

    bld = Builder()
    if args.scene == "sphere":
        shader = bld.NewSphere(1.0)
    elif args.scene == "text-plate":
        # BASELINE configs[4]'s tree from the reference's own font (forge/textsdf mirror over tests/golden/iso-3098.ttf, the data
        # file forge/textsdf/embed.go embeds): TextLine -> Extrude -> Union with a base plate (examples/ui-text/uitext.go:30-42)
        ttf = open(os.path.join(ROOT, "tests", "golden", "iso-3098.ttf"), "rb").read()
        t2 = bld.TextLine(ttf, "gsdf MI355X")
        tb = t2.Bounds()
        w, h = float(tb[3] - tb[0]), float(tb[4] - tb[1])
        plate = bld.Translate(bld.NewBox(w + 0.3, h + 0.3, 0.06, 0.01), float(tb[0] + tb[3]) / 2, float(tb[1] + tb[4]) / 2, -0.08)
        shader = bld.Union(bld.Extrude(t2, 0.12), plate)
    else:
        shader = bld.Scene(args.scene)
    res = np.float32(float(shader.Diagonal()) / args.resdiv)
    sdf = hip.SDF3HIP(shader)
    spec_note = "interpreter kernels"
    if not args.interpreter:
        # per-tree kernel build (hiprtc), outside the timed region: the analogue of the reference compiling its GLSL
        # compute shader for the tree (gleval/gpu.go:35-54). --interpreter keeps the generic interpreter kernels, which
        # also remain in use if the run-time build is not possible on this box (still the HIP path, same bits).
        try:
            sdf.specialize()
            inf = sdf.info()
            spec_note = "kernels specialised for the tree at setup (%s, %.1f s, untimed)" % (inf["kernels"].get("compiler", "hiprtc"), inf["specialize_s"])
        except hip.HipError as e:
            print("bench: specialised build unavailable, using the interpreter kernels: %s" % str(e)[:300], file=sys.stderr)
            spec_note = "interpreter kernels (specialised build failed)"

    # Dual contouring's meshes are one blocking chain each, with host round trips between its stages (the octree's second and third
    # workspace have no counterpart there): a caller with several meshes to make keeps the GPU busy the way a Go caller would --
    # a second handle of the same tree and a host thread per handle (N = 1; --no-mesh-pipeline: one handle, one mesh at a time).
    sdf_b = None  # (a list of the further handles, or None)
    if args.mode == "mesh" and args.renderer == "dualcontour" and world == 1 and not args.no_mesh_pipeline and not force_dist and args.dc_handles > 1:
        sdf_b = []
        for _ in range(args.dc_handles - 1):
            hb = hip.SDF3HIP(shader)
            if not args.interpreter and "specialised" in spec_note:
                try:
                    hb.specialize()
                except hip.HipError:
                    pass  # (this handle keeps the interpreter kernels: same bits)
            sdf_b.append(hb)

    if args.mode == "eval":
        return eval_mode(args, torch, np, hip, shader, sdf, res, dev)
    if args.mode == "flat":
        return flat_mode(args, torch, np, hip, shader, sdf, res, spec_note)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    GM = {"all": hip.GATHER_ALL, "root": hip.GATHER_ROOT, "none": hip.GATHER_NONE}
    pipeline = comm is not None and not args.no_gather_pipeline
    dc = args.renderer == "dualcontour"
    G = {}  # the gather of the loop being run (use_gather): mode, what moves, the payload constant

    def use_gather(mode):
        # what moves in the gather: packed cut-leaf records by default (marching cubes then runs on the receiving ranks)
        G["mode"] = mode
        G["records"] = (comm is not None and args.payload == "records" and mode != "none" and not dc)
        G["payload"] = hip.PAYLOAD_RECORDS if G["records"] else hip.PAYLOAD_TRIANGLES
    use_gather(args.gather)
    gstat = {"n": 0, "ms_counts": 0.0, "ms_payload": 0.0, "ms_march": 0.0, "bytes_received": 0, "bytes_sent": 0}
    pending = []  # at most one gather in flight: (PendingGather)

    def finish():
        g = None
        while pending:
            g, _, gs = pending.pop(0).wait()
            gstat["n"] += 1
            gstat["ms_counts"] += gs.ms_counts
            gstat["ms_payload"] += gs.ms_payload
            gstat["ms_march"] += gs.ms_march
            gstat["bytes_received"] += gs.bytes_received
            gstat["bytes_sent"] += gs.bytes_sent
        return g

    def step():
        if dc:  # BASELINE configs[4]: dual contouring, z-slabs of the lattice per rank
            oc = hip.DualContourHIP(sdf, res, shard_rank=rank, shard_count=world)
        else:
            oc = hip.OctreeHIP(sdf, res, shard_rank=rank, shard_count=world, share_corners=args.share_corners, payload=G["payload"])
        gathered = None
        if comm is not None:
            # the counts are exchanged and the payload enqueued on the communicator's stream; with the pipeline on, the
            # previous mesh's payload is awaited only now, i.e. it moved while this mesh was made
            pg = oc.gatherv_start(comm, GM[G["mode"]], 0)
            gathered = finish()
            pending.append(pg)
            if not pipeline:
                gathered = finish()
        elif torch_gather:
            from gsdf_amd.gather import all_gatherv_triangles
            gathered = all_gatherv_triangles(oc.dev_ptr(), oc.n_tris(), dev)[0]
        return oc, gathered

    # Setup, untimed: bring the GPU out of its idle clock state before the W warmup steps. The first ~20 meshes after
    # start-up run 5 % slower (1.70 vs 1.61 ms leaf kernel), and with the contract's small W they would be the ones timed.
    mesh_pipeline = (comm is None and not torch_gather and not dc and not args.no_mesh_pipeline)
    rank_pipeline = (comm is not None and not dc and not args.no_mesh_pipeline)  # the N > 1 form of it (run_meshes)

    def run_meshes(n, account=None, sc=None):
        """n meshes, every one started and finished inside this call. Pipelined (N = 1): up to --mesh-depth meshes are in flight -- the
        chains of kernels of meshes k + 1 (and k + 2) are enqueued, on the handle's other workspaces and streams, before mesh k is waited for."""
        last = None
        sc = args.share_corners if sc is None else sc
        if dc and sdf_b is not None:
            return run_dc_two_handles(n, account)
        if rank_pipeline:
            # N > 1 over the library's gather: the same pipeline of meshes on every rank -- a rank's shard is an eighth of a third of a
            # millisecond, a blocking mesh there is all latency (the replicated top levels, a dozen dependent launches) -- and the
            # payload of mesh k moves on the communicator's stream while meshes k + 1 .. are made, as in step()
            inflight, started = [], 0
            for k in range(n):
                while started < n and len(inflight) < args.mesh_depth:
                    inflight.append(hip.OctreeHIP.start(sdf, res, shard_rank=rank, shard_count=world, share_corners=sc, payload=G["payload"]))
                    started += 1
                oc = inflight.pop(0).wait()
                pg = oc.gatherv_start(comm, GM[G["mode"]], 0)
                gathered = finish()
                pending.append(pg)
                if not pipeline:
                    gathered = finish()
                last = (oc, gathered)
                if account:
                    account(oc)
            return last
        if not mesh_pipeline:
            for _ in range(n):
                last = step()
                if account:
                    account(last[0])
            return last
        inflight = []  # args.mesh_depth meshes in flight: the handle's workspaces and streams (three)
        started = 0
        for k in range(n):
            while started < n and len(inflight) < args.mesh_depth:
                inflight.append(hip.OctreeHIP.start(sdf, res, share_corners=sc))
                started += 1
            last = (inflight.pop(0).wait(), None)
            if account:
                account(last[0])
        return last

    def run_dc_two_handles(n, account):
        """n dual-contouring meshes, every one made inside this call: handle t of H makes meshes t, t + H, ... in its own host thread (the C calls
        release the GIL); a mesh is accounted and let go as soon as it is done, the last one is kept."""
        import threading
        lock, keep, errs = threading.Lock(), {}, []
        handles = [sdf] + list(sdf_b)

        def worker(t):
            try:
                for i in range(t, n, len(handles)):
                    oc = hip.DualContourHIP(handles[t], res, shard_rank=rank, shard_count=world)
                    with lock:
                        if account:
                            account(oc)
                        keep[i] = oc if i == n - 1 else None
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(len(handles))]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        if errs:
            raise errs[0]
        return (keep.get(n - 1), None) if n > 0 else None

    def timed_loop():
        """The contract's loop for the gather in use: W untimed steps, then EXACTLY K steps between barrier + synchronize on both sides;
        the time is the maximum over the ranks, evaluations and triangles the sums."""
        run_meshes(args.warmup)
        finish()
        for k in gstat:
            gstat[k] = 0
        acc = {"evals": 0, "tris": 0, "march_ms": 0.0, "march_evals": 0.0, "march_tris": 0.0, "emit_ms": 0.0, "cut": 0.0}

        trace = [] if os.environ.get("GSDF_BENCH_STEP_TRACE") else None  # developer: wall clock at every finished step -> the largest gaps on stderr

        def account(oc):
            st = oc.stats
            if trace is not None:
                trace.append(time.perf_counter())
            acc["evals"] += st.evals
            acc["tris"] += st.n_tris
            acc["march_ms"] += st.ms_march
            acc["march_evals"] += st.evals_leaf
            acc["march_tris"] += st.n_tris
            acc["emit_ms"] += st.ms_emit
            acc["cut"] += st.cut_leaves

        import gc
        gcmode = os.environ.get("GSDF_BENCH_GC", "")  # developer experiment (HISTORY round 6, item 18): "freeze" / "disable" / "collect"; default: nothing
        if gcmode in ("freeze", "collect", "disable"):
            gc.collect()
        if gcmode == "freeze":
            gc.freeze()
        if gcmode == "disable":
            gc.disable()
        barrier()
        t0 = time.perf_counter()
        last = run_meshes(args.steps, account)
        gl = finish()  # the last mesh's gather belongs to the timed region too
        if gl is not None:
            last = (last[0], gl)
        barrier()
        dt = time.perf_counter() - t0
        gc.enable()
        if trace is not None and len(trace) > 2:
            gaps = sorted(((trace[i + 1] - trace[i]) * 1e3, i) for i in range(len(trace) - 1))
            print("bench: step trace: median gap %.4f ms, largest %s, gc counts %s" % (gaps[len(gaps) // 2][0], [(round(g, 3), i) for g, i in gaps[-6:]], gc.get_count()), file=sys.stderr)
        tot = torch.tensor([float(acc["evals"]), float(acc["tris"]), dt], dtype=torch.float64, device=dev if torch_gather else "cpu")
        evals_minmax = None
        if dist is not None:
            tmax = tot.clone()
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax[2])
            # load balance of the brick partition: evaluations per step of the least and the most loaded rank
            lo = torch.tensor([float(acc["evals"])], dtype=torch.float64, device=tot.device)
            hi = lo.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            evals_minmax = (float(lo[0]) / args.steps, float(hi[0]) / args.steps)
        r = {"last": last, "acc": acc, "dt": dt, "evals_all": float(tot[0]), "tris_all": float(tot[1]), "evals_minmax": evals_minmax,
             "gstat": dict(gstat), "mode": G["mode"], "records": G["records"]}
        if dist is not None and rank == 0 and last[1] is not None:
            ng = last[1].n_tris() if hasattr(last[1], "n_tris") else int(last[1].shape[0])
            assert ng == int(r["tris_all"] / args.steps), "gathered triangle count differs from the sum of the ranks'"
        return r

    def gather_report(r):
        """One timed loop's gather as the line reports it (rank 0's HIP events on the communicator's stream)."""
        gs, n = r["gstat"], max(1, r["gstat"]["n"])
        step_ms = r["dt"] / args.steps * 1e3
        g_ms = (gs["ms_counts"] + gs["ms_payload"] + gs["ms_march"]) / n
        st = r["last"][0].stats
        return {"mode": r["mode"], "pipelined": pipeline, "payload": "records" if r["records"] else "triangles",
                "transport": comm.transport(), "ms_per_step": step_ms, "evals_per_s": r["evals_all"] / r["dt"], "triangles_per_s": r["tris_all"] / r["dt"],
                "bytes_received_per_rank": gs["bytes_received"] / n, "bytes_sent_per_rank": gs["bytes_sent"] / n, "ms": g_ms,
                "ms_counts": gs["ms_counts"] / n, "ms_payload": gs["ms_payload"] / n, "ms_march_after_gather": gs["ms_march"] / n,
                "evals_per_step_min_max_over_ranks": r["evals_minmax"],
                # how much of the shorter of the two (meshing on the device, gather on the wire) hid behind the other
                "overlap_frac": max(0.0, min(1.0, (st.ms_total + g_ms - step_ms) / max(1e-9, min(st.ms_total, g_ms))))}

    run_meshes(args.preheat)
    H = timed_loop()  # the headline: the gather mode --gather names (default all)
    if args.dump_outputs:
        if rank == 0:  # what rank 0's caller holds after the last step: the gathered mesh, or its own (gather none, N = 1)
            lo, lg = H["last"]
            dump_outputs(args.dump_outputs, mesh_outputs(lg if lg is not None else lo, lo.stats.evals))
        if dist is not None:
            barrier()
    gather_modes = None
    if comm is not None:
        # Beside the headline, after it: the SAME loop with the other two gather modes, so that one N > 1 run separates what the
        # compute scales to (none: every rank keeps its shard) from what the wire allows (root, all) -- xGMI is one ~60 GB/s link per
        # peer, one GPU emits triangles at 400 GB/s
        gather_modes = {args.gather: gather_report(H)}
        if args.full and not args.no_gather_modes:
            for mode in ("all", "root", "none"):
                if mode != args.gather:
                    use_gather(mode)
                    gather_modes[mode] = gather_report(timed_loop())
            use_gather(args.gather)
    last, dt, evals_all, tris_all = H["last"], H["dt"], H["evals_all"], H["tris_all"]
    evals, tris, march_ms, march_evals, march_tris, emit_ms, cut = (H["acc"][k] for k in ("evals", "tris", "march_ms", "march_evals", "march_tris", "emit_ms", "cut"))
    records = H["records"]

    # The dominant kernel ALONE, after the timed loops: blocking meshes of rank 0's shard with the device to itself (the other
    # ranks wait at the barrier -- they may share rank 0's device), no gather. Every --full line takes its roofline from these.
    alone = None
    if args.full:
        barrier()
        if rank == 0 and not dc:
            alone = [hip.OctreeHIP(sdf, res, shard_rank=rank, shard_count=world, share_corners=args.share_corners).stats for _ in range(8)][2:]
        elif rank == 0:
            alone = [hip.DualContourHIP(sdf, res, shard_rank=rank, shard_count=world) for _ in range(4)][1:]
            alone_stage_ms = [a.stage_ms() for a in alone]
        barrier()

    if rank == 0:
        oc, g = last
        st = oc.stats
        workload = (f"examples/{args.scene} resdiv {args.resdiv}: "
                    + ("dual contouring (least-squares vertex placement) on device " if dc else "octree prune + marching cubes on device ")
                    + f"(res {float(res):.7f}, {st.levels} levels)")
        kern = sdf.info()["kernels"]
        code = kern.get("code")
        dc_stages = rf = None
        two_kernel = emit_ms > 0 or (alone is not None and not dc and alone[0].ms_emit > 0)  # leaf phase = leaf_eval_kernel (dominant) + march_records_kernel
        if alone is None:
            pass  # (plain run: the roofline objects take runs of their own, --full)
        elif dc:
            # five stages, timed apart by HIP events (gsdf_hip_mesh_stage_ms): the roofline is the longest one's
            sm = {k: sum(a[k] for a in alone_stage_ms) / len(alone_stage_ms) for k in alone_stage_ms[0]}
            nc, ne, nq, no = float(st.leaf_cubes), float(st.active_leaves), float(st.n_tris) / 2, float(st.evals_prune)
            alg = {"dc_origin": 16.0 * no + 4.0 * no,            # position + distance per evaluated cell, + its index-grid word
                   "dc_edges": 16.0 * 4 * nc + 8.0 * nc + 28.0 * nc + 4.0 * ne,  # 4 evaluations per kept cube, its cube word in, distances + default vertex out, an edge word per active edge
                   "dc_normals": 16.0 * 6 * ne + 36.0 * ne,       # 6 evaluations per active edge (central differences), crossing + normal out
                   "dc_place": (16.0 + 8.0 + 12.0) * nc + 36.0 * ne,  # distances, cube word, vertex out; the crossings / normals of its edges in
                   "dc_quads": 72.0 * nq + 4.0 * ne + 4 * 12.0 * nq}  # two triangles out per quad, four vertices + an edge word in
            dc_stages = {k: {"ms": v, "algorithmic_gb": alg[k] / 1e9, "gb_per_s": alg[k] / 1e9 / (v * 1e-3) if v > 0 else 0.0} for k, v in sm.items()}
            kmax = max(sm, key=sm.get)
            pm_st, pm_match = pmc_dc_stages(workload, code)
            for k, v in pm_st.items():  # counters of the same kernels, if a summary under profiles/ carries this workload
                dc_stages.setdefault(k, {})["pmc"] = v
            vi = (pm_st.get(kmax) or {}).get("SQ_INSTS_VALU")
            ach = (vi * 64 / (sm[kmax] * 1e-3)) if (vi and world == 1) else None
            rf = {"bound": "valu", "kernel": kmax + "_kernel (the longest of the five stages; all of them under 'stages')", "kernel_ms": sm[kmax],
                  "achieved": ach / 1e12 if ach else None, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "T lane-instr/s",
                  "frac": ach / VALU_PEAK_LANE_OPS if ach else None, "traffic": (pm_st.get(kmax) or {}).get("hbm_traffic_gb_per_launch"),
                  "traffic_unit": "GB per launch (PMC: 2*FETCH_SIZE + WRITE_SIZE)",
                  "counters": counters_note((pm_st.get(kmax) or {}).get("counters_from"), pm_match),
                  "hbm_notional": {"algorithmic_gb_per_launch": alg[kmax] / 1e9, "gb_per_s": dc_stages[kmax]["gb_per_s"], "peak": HBM_PEAK_GBS, "unit": "GB/s"},
                  "note": "stage times of blocking meshes after the timed loop; achieved = SQ_INSTS_VALU x 64 lanes of that stage's kernel (PMC summary) / its time"}
        else:
            # ALGORITHMIC bytes of the dominant kernel: 16 B per evaluation it performs (12 B position + 4 B distance;
            # positions are generated on device but counted); the evaluating kernel of the two-kernel leaf phase hands 40-byte
            # cut-leaf records on, the fused kernel emits the triangles (36 B each). Notional by construction: the kernel moves 6 %
            # of that (PMC traffic) -- so it is reported as bytes and GB/s, never as a fraction of the HBM peak.
            a_ms = sum(a.ms_march for a in alone) / len(alone)
            a_ev = sum(a.evals_leaf for a in alone) / len(alone)
            a_cut = sum(a.cut_leaves for a in alone) / len(alone)
            a_tri = sum(a.n_tris for a in alone) / len(alone)
            k_bytes = a_ev * 16.0 + (a_cut * 40.0 if two_kernel else a_tri * 36.0)
            kernel_rate = a_ev / (a_ms * 1e-3) if a_ms > 0 else 0.0
            va = valu_roofline(kernel_rate, workload, code)
            pm = pmc_summary(workload, code)
            rf = {"bound": "valu", "kernel": kern.get("leaf", "leaf_kernel"), "kernel_ms": a_ms,
                  "achieved": va["achieved"] if va else None, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "T lane-instr/s",
                  "frac": va["frac"] if va else None, "traffic": pm.get("hbm_traffic_gb_per_launch"), "traffic_unit": "GB per launch (PMC: 2*FETCH_SIZE + WRITE_SIZE)",
                  "counters": counters_note(pm.get("source"), pm.get("code_match")),
                  "kernel_evals_per_s": kernel_rate, "kernel_span_in_loop_ms": march_ms / max(1, args.steps),
                  "ms_per_mesh_device_alone": sum(a.ms_total for a in alone) / len(alone), "valu": va,
                  "hbm_notional": {"algorithmic_gb_per_launch": k_bytes / 1e9, "gb_per_s_alone": k_bytes / (a_ms * 1e-3) / 1e9 if a_ms > 0 else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "note": "16 B per evaluation + 40 B per cut-leaf record, as SURVEY 8(d) counts them; positions are generated in registers and distances never "
                                           "leave the CU, so these bytes do not cross HBM (roofline.traffic does) and no fraction of the HBM peak is formed from them"},
                  "note": ("bound by VALU issue (SURVEY 8(d)): achieved = SQ_INSTS_VALU x 64 lanes per evaluation (PMC summary under profiles/, see `counters`) x the kernel's "
                           "evaluations per second with the GPU to itself (blocking meshes of rank 0's shard after the timed loop, HIP events on the launching stream); peak = 256 CUs x "
                           "4 SIMDs x 32 lanes x 2.4 GHz; valu.mix_roof_frac prices the same rate against what the kernel's own instruction mix allows on gfx950 "
                           "(tools/ubench/class_rate.hip); kernel_span_in_loop_ms is the kernel's event-to-event span inside the timed loop"
                           + (", where it shares the CUs with the other mesh in flight" if mesh_pipeline else ""))}
        out = {
            "schema": 6,
            "metric": "sdf_evals_per_s", "value": evals_all / dt, "unit": "evals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "evaluator_build": "interpreter" if (args.interpreter or "specialised" not in spec_note) else "specialised",
            "config": {"workload": workload,
                       "sharding": (("z-slabs of the lattice, halo recomputed" if dc else "octree bricks by coordinate hash")
                                    + ((", gather of " + ("packed cut-leaf records (marching cubes after the gather)" if records else "triangles") + " inside the library over " + comm.transport() + " (gsdf_hip_mesh_gatherv_start/_wait): mode " + args.gather
                                        + (", payload of mesh i overlapped with mesh i+1" if pipeline else ", not pipelined")) if comm is not None else ", RCCL all-gatherv of triangles through torch.distributed (fallback)")) if (world > 1 or comm is not None) else "single GPU",
                       "leaf_corners": {0: "8 per leaf (as the reference)", 1: "shared (distinct lattice points once)",
                                        2: "the bitwise-distinct z rows of a brick once each (evals_per_step counts the evaluations performed)",
                                        3: "distinct lattice points or distinct z rows of a brick once each, chosen by the library for the tree (evals_per_step counts the evaluations performed)"}[args.share_corners],
                       "evaluator": spec_note, "code": code,
                       "setup": f"{args.preheat} untimed meshes before the warmup steps (clock ramp)",
                       "steps": (f"meshes pipelined {args.mesh_depth} deep on one handle (gsdf_hip_mesh_octree_start / _wait): the kernels of the next meshes are enqueued before mesh k "
                                 "is waited for; all K started and finished inside the timed region") if mesh_pipeline else
                                (f"{args.dc_handles} handles of the tree, a host thread and one blocking dual-contouring mesh in flight on each (a mesh is one chain with host round trips "
                                 "between its stages); all K made inside the timed region; --no-mesh-pipeline: one handle, one mesh at a time") if (dc and sdf_b is not None)
                                else (f"every rank: its shard's meshes pipelined {args.mesh_depth} deep on one handle (gsdf_hip_mesh_octree_start / _wait), the gather of mesh k started when "
                                      "mesh k is done; all K started, finished and gathered inside the timed region") if rank_pipeline
                                else "one blocking mesh call per step"},
            "triangles_per_s": tris_all / dt,
            "triangles_per_step": tris_all / args.steps, "evals_per_step": evals_all / args.steps,
            "phase_ms_rank0": {"prune": st.ms_prune, "leaf": st.ms_leaf, "eval_kernel": st.ms_march, "march_kernel": st.ms_emit, "total_device": st.ms_total},
            "phase_note": ("event-to-event spans of the timed loop's LAST mesh" + (": it shares the device with the other mesh in flight, so the spans overlap the other chain's kernels "
                           "(a mesh with the device to itself: roofline.ms_per_mesh_device_alone, --full)" if mesh_pipeline else "")),
            "full": args.full,
        }
        if args.full:
            out["roofline"] = rf
            out["stages"] = dc_stages
        if args.full and not dc and two_kernel:
            # march_records_kernel alone (the same blocking meshes): its two streams against the HBM peak and against what a plain
            # HIP copy kernel of as many bytes reaches on this part (tools/ubench/copy_rate.hip; profiles/r6m_copy_rate.txt)
            m_ms = sum(a.ms_emit for a in alone) / len(alone)
            e_bytes = a_cut * 40.0 + a_tri * 36.0
            m_gbs = e_bytes / (m_ms * 1e-3) / 1e9 if m_ms > 0 else 0.0
            cr = guarded(copy_rate_gbs, a_cut * 40.0, a_tri * 36.0)
            cr_gbs = (cr or {}).get("gb_per_s")
            out["roofline_march"] = {"bound": "hbm", "kernel": "march_records_kernel", "kernel_ms": m_ms, "algorithmic_gb_per_launch": e_bytes / 1e9,
                                     "achieved": m_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": m_gbs / HBM_PEAK_GBS,
                                     "frac_of_copy": m_gbs / cr_gbs if cr_gbs else None, "copy": cr,
                                     "kernel_span_in_loop_ms": emit_ms / max(1, args.steps),
                                     "note": "marching cubes over the cut-leaf records, kernel alone: 40 B read per record + 36 B written per triangle; frac_of_copy = against the "
                                             "rate a 16-B-per-lane HIP copy kernel reading and writing the same byte counts reaches on this box in this run (tools/ubench/copy_rate.hip)"}
        if shared_device:
            out["config"]["devices"] = (f"{world} ranks on {ndev} GPU(s): ranks share a device over the library's inter-process transport (GSDF_HIP_COMM=ipc) -- "
                                        "the N > 1 code path end to end, not a scaling measurement")
        if args.full and mesh_pipeline and not dc and args.share_corners == 0 and not args.no_distinct_rows:
            # Beside the headline, not in it: the same mesh with the evaluations the reference repeats left out (gsdf_mesh_opts.share_corners;
            # the triangle set is bit-identical, tests/test_gpu_mesh.py) -- time to mesh for a caller who does not need the reference's
            # evaluation count. Same pipelined loop, after the timed region. 2: every bitwise-distinct z row of a brick once (the
            # headline's kernels); 1: every bitwise-distinct lattice point of a brick once (leaf_dense_kernel: no column sharing).
            def shared(sc, key):
                run_meshes(max(5, args.preheat // 2), sc=sc)  # (its own kernels; the clocks have relaxed during the blocking meshes above)
                dacc = {"evals": 0, "tris": 0}
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                run_meshes(args.steps, lambda o: (dacc.__setitem__("evals", dacc["evals"] + o.stats.evals), dacc.__setitem__("tris", dacc["tris"] + o.stats.n_tris)), sc=sc)
                torch.cuda.synchronize()
                dt2 = time.perf_counter() - t1
                al2 = [hip.OctreeHIP(sdf, res, share_corners=sc).stats for _ in range(8)][2:]
                return {"ms_per_step": dt2 / args.steps * 1e3, "triangles_per_s": dacc["tris"] / dt2, "triangles_per_step": dacc["tris"] / args.steps,
                        "evals_performed_per_step": dacc["evals"] / args.steps, "evals_performed_per_s": dacc["evals"] / dt2,
                        "reference_evals_per_s": evals_all / dt2, "kernel": sdf.info()["kernels"].get(key),
                        "alone": {"kernel_ms": sum(a.ms_march for a in al2) / len(al2), "ms_per_mesh_device": sum(a.ms_total for a in al2) / len(al2)}}
            for key_, sc_, kern_ in (("distinct_rows", 2, "leaf_rows"), ("distinct_points", 1, "leaf_dense")):
                try:  # (an option beside the headline must never cost the headline its line)
                    out[key_] = shared(sc_, kern_)
                except Exception as ex:  # noqa: BLE001
                    out[key_] = {"error": repr(ex)[:300]}
            out["distinct_rows"]["note"] = ("gsdf_mesh_opts.share_corners = 2: rows 2k-1 and 2k of a brick's eight z rows of corners are the same plane and mostly the same float; "
                                            "each distinct row is evaluated once. Bit-identical triangle set; not the headline, which performs every evaluation the reference performs")
            out["distinct_points"]["note"] = ("gsdf_mesh_opts.share_corners = 1: every bitwise-distinct lattice point of a brick once (5..8 coordinates per axis instead of 8), packed "
                                              "four to a lane, no (x, y) column sharing; evals_performed counts lane slots. Bit-identical triangle set; not the headline")
        if gather_modes:
            gh = gather_modes[args.gather]
            out["phase_ms_rank0"]["gather_counts"] = gh["ms_counts"]
            out["phase_ms_rank0"]["gather"] = gh["ms_payload"]
            out["phase_ms_rank0"]["gather_march"] = gh["ms_march_after_gather"]
            out["gather"] = dict(gh, note="rank 0, HIP events on the communicator's stream; a step = one mesh + its gather")
        if gather_modes and args.full:
            out["gather_modes"] = dict(gather_modes, note="the same K-step loop once per mode, one after the other in this run; the headline (`value`, `ms_per_step`) is mode "
                                       + args.gather + "; `none` is what the compute scales to, `root` / `all` add the wire")
        if args.full and world == 1 and comm is None and not dc:
            out["host_inclusive"] = guarded(host_inclusive, hip, sdf, res)
        if args.full and world == 1 and comm is None and not dc and not args.no_evaluate_dropin and args.scene != "text-plate":
            out["evaluate_dropin"] = guarded(evaluate_dropin, hip, sdf, shader)
        if args.full and world == 1 and comm is None and not dc and not args.no_one_shot and not args.interpreter:
            out["one_shot"] = guarded(one_shot, hip, shader, res)
        # (last: its 255 host threads leave the host's clocks and caches in a state the host-side measurements above should not see)
        if args.full and world == 1 and not args.no_cpu_baseline and not dc:
            threads = max(1, (os.cpu_count() or 2) - 1)  # GOMAXPROCS-1 (gsdfaux/gsdfaux.go:162-164)
            # bounded sample of the SAME workload: full resdiv 1600 lattice (420 M evals) on big hosts, coarser on small ones
            cpu_rd = args.cpu_resdiv or (args.resdiv if threads >= 64 else (1000 if threads >= 16 else 600))
            out["cpu_baseline"] = guarded(cpu_baseline, shader, args.scene, cpu_rd, threads)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        if comm is not None:
            comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
