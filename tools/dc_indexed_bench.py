#!/usr/bin/env python3
"""What dual contouring straight to an indexed mesh costs, beside the soup and beside the only other way to the same handle: one
JSON line per config (profiles/dc_indexed_bench.jsonl).

    python tools/dc_indexed_bench.py [--reps 7] [--warmup 2] [--resdiv 800]

The text plate and npt-flange at resdiv 800, per-tree kernels -- the dual-contouring configs DESIGN.md section 8 quotes. Three
things are timed per config, alternating within one repetition so that the machine's drift falls on all three alike:
  (a) soup       gsdf_hip_mesh_dualcontour alone
  (b) indexed    gsdf_hip_mesh_dualcontour_indexed
  (c) host_weld  the soup route to the same handle: gsdf_hip_mesh_dualcontour, gsdf_hip_mesh_host_tris (D2H), numpy.unique over
                 the corners on the host, gsdf_hip_indexed_create (H2D); its parts are reported too
Two kinds of time, never mixed in one difference:
  *_wall_ms    the host clock around the blocking call(s); what `indexed_minus_soup_wall_ms` and the ratios compare
  *_device_ms  HIP events inside the library: the meshers' ms_total, the new stage's ms_keys (quads into lattice order) and
               ms_number (owners, numbering, gather, index write). soup_device_ms, ms_keys and ms_number are device time alone;
               indexed_device_ms is the indexed entry's ms_total, whose interval holds one wait for the host (the quad count) and
               ends before the numbering: an event interval, not a sum of kernel times
bytes_per_quad: what the new stage moves per quad by its own accounting (kernels_dc_indexed.h: 20 + 12 + 48 in the ordering passes,
24 + 24 + 24 + 20 in the numbering: idx read by cube_first, topo_owner, cube_number and rewritten by remap, plus a vertex's 20 bytes for
about every second quad) against the soup's 72 written. Median of the repetitions after the warm-up; min and max beside it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text_plate(bld):
    """bench.py's --scene text-plate."""
    ttf = open(os.path.join(ROOT, "tests", "golden", "iso-3098.ttf"), "rb").read()
    t2 = bld.TextLine(ttf, "gsdf MI355X")
    tb = t2.Bounds()
    w, h = float(tb[3] - tb[0]), float(tb[4] - tb[1])
    plate = bld.Translate(bld.NewBox(w + 0.3, h + 0.3, 0.06, 0.01), float(tb[0] + tb[3]) / 2, float(tb[1] + tb[4]) / 2, -0.08)
    return bld.Union(bld.Extrude(t2, 0.12), plate)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resdiv", type=int, default=800)
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    args = ap.parse_args(argv)
    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    for scene in ("text-plate", "npt-flange"):
        bld = Builder()
        shape = text_plate(bld) if scene == "text-plate" else bld.Scene(scene)
        res = np.float32(float(shape.Diagonal()) / args.resdiv)
        sdf = hip.SDF3HIP(shape)
        if not args.interpreter:
            sdf.specialize()
        t = {k: [] for k in ("soup_wall", "soup_dev", "ix_wall", "ix_dev", "keys", "number", "host_wall", "host_mesh", "host_d2h", "host_unique", "host_create")}
        last = None
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            dc = hip.DualContourHIP(sdf, res)
            t1 = time.perf_counter()
            ix = hip.IndexedHIP.dual_contour(sdf, res)
            t2 = time.perf_counter()
            dc2 = hip.DualContourHIP(sdf, res)
            t3 = time.perf_counter()
            tris = dc2.triangles_view()
            t4 = time.perf_counter()
            uniq, inv = np.unique(tris.reshape(-1, 3).view(np.dtype((np.void, 12))).reshape(-1), return_inverse=True)
            verts = uniq.view(np.float32).reshape(-1, 3)
            t5 = time.perf_counter()
            hx = hip.IndexedHIP.from_arrays(verts, inv.reshape(-1, 3).astype(np.uint32))
            t6 = time.perf_counter()
            if k >= args.warmup:
                st = ix.stats
                for key, v in (("soup_wall", (t1 - t0) * 1e3), ("soup_dev", dc.stats.ms_total), ("ix_wall", (t2 - t1) * 1e3), ("ix_dev", ix.mesh_stats.ms_total),
                               ("keys", st.ms_keys), ("number", st.ms_number), ("host_wall", (t6 - t2) * 1e3), ("host_mesh", (t3 - t2) * 1e3),
                               ("host_d2h", (t4 - t3) * 1e3), ("host_unique", (t5 - t4) * 1e3), ("host_create", (t6 - t5) * 1e3)):
                    t[key].append(float(v))
            last = (dc, ix, hx)
            del tris
        dc, ix, hx = last
        assert ix.n_tris == dc.n_tris() == hx.n_tris, (ix.n_tris, dc.n_tris(), hx.n_tris)
        quads = ix.n_tris // 2
        m = {k: spread(v) for k, v in t.items()}
        line = {"scene": scene, "resdiv": args.resdiv, "res": float(res), "form": "interpreter" if args.interpreter else "specialised",
                "levels": int(ix.mesh_stats.levels), "kept_cubes": int(ix.mesh_stats.leaf_cubes), "active_edges": int(ix.mesh_stats.active_leaves),
                "quads": quads, "n_tris": ix.n_tris, "n_verts": ix.n_verts, "host_weld_n_verts": hx.n_verts,  # (by position: two cubes may place their vertices on one point)
                "soup_wall_ms": m["soup_wall"], "soup_device_ms": m["soup_dev"], "indexed_wall_ms": m["ix_wall"], "indexed_device_ms": m["ix_dev"],
                "ms_keys": m["keys"], "ms_number": m["number"],
                "indexed_minus_soup_wall_ms": m["ix_wall"]["median"] - m["soup_wall"]["median"],
                "indexed_minus_soup_over_soup": (m["ix_wall"]["median"] - m["soup_wall"]["median"]) / m["soup_wall"]["median"],
                "host_weld_wall_ms": m["host_wall"], "host_weld_parts_ms": {"mesh": m["host_mesh"], "d2h": m["host_d2h"], "unique": m["host_unique"], "create": m["host_create"]},
                "host_weld_over_indexed": m["host_wall"]["median"] / m["ix_wall"]["median"],
                "bytes_per_quad": {"order": 80, "number": 72 + 20.0 * ix.n_verts / quads, "soup_written": 72},
                "new_stage_bytes_per_s": quads * (152 + 20.0 * ix.n_verts / quads) / ((m["keys"]["median"] + m["number"]["median"]) * 1e-3),
                "reps": args.reps, "warmup": args.warmup}
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
