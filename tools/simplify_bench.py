#!/usr/bin/env python3
"""Timing of gsdf_hip_indexed_simplify (kernels_simplify.h) on the GPU against the weld of the same mesh.

For npt-flange at each `--resdivs` and each cell of `--cells` x res (grid half a res below the mesh's lattice origin, as examples/render_ply.py): after `--warmup` calls the
MEDIAN over `--reps` calls of the stats' own HIP-event times (ms_cells, ms_faces) and of a dry run's, attempts, largest cluster,
triangles in and out, and the unsigned relative change of the report's volume and area against the unsimplified mesh; the weld's
device time (median over the same number of welds of the same records) is the yardstick. One JSON line per measurement. Kernel times:
run this under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/simplify_bench.py [--scene npt-flange] [--resdivs 400,1600] [--cells 2,4,8] [--reps 9] [--warmup 2] [-o lines.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="npt-flange")
    ap.add_argument("--resdivs", default="400,1600")
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)

    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    shape = Builder().Scene(args.scene)
    sdf = hip.SDF3HIP(shape)
    lines = []
    med = statistics.median
    for resdiv in [int(x) for x in args.resdivs.split(",")]:
        res = np.float32(float(shape.Diagonal()) / resdiv)
        mesh = hip.OctreeHIP(sdf, res, payload=hip.PAYLOAD_RECORDS)
        origin = tuple(np.float32(o) - np.float32(0.5) * res for o in mesh.stats.origin[:])  # as examples/render_ply.py: no lattice plane is a cell face
        welds = [mesh.weld() for _ in range(args.warmup + args.reps)]
        weld_ms = med(w.ms_device for w in welds[args.warmup:])
        ix = welds[-1]
        del welds
        rep = ix.report()
        for k in [float(x) for x in args.cells.split(",")]:
            cell = np.float32(k) * res
            runs, dries = [], []
            for n in range(args.warmup + args.reps):
                out, st = ix.simplify(cell, origin)
                _, sd = ix.simplify(cell, origin, dry=True)
                if n >= args.warmup:
                    runs.append(st)
                    dries.append(sd)
            r2 = out.report()
            st = runs[-1]
            lines.append({"scene": args.scene, "resdiv": resdiv, "cell_res": k, "n_tris_in": int(st.n_tris_in), "n_tris": int(st.n_tris),
                          "n_verts_in": int(st.n_verts_in), "n_verts": int(st.n_verts), "cells": int(st.cells), "collapsed": int(st.collapsed),
                          "largest_cell": int(st.largest_cell), "attempts": int(st.attempts), "probes": int(st.probes), "table_cells": int(st.table_cells),
                          "ms_cells": med(s.ms_cells for s in runs), "ms_faces": med(s.ms_faces for s in runs),
                          "ms_total": med(s.ms_cells + s.ms_faces for s in runs),
                          "dry_ms_total": med(s.ms_cells + s.ms_faces for s in dries), "weld_ms_device": weld_ms,
                          "volume": rep.volume, "volume_simplified": r2.volume, "volume_rel_change": abs(r2.volume - rep.volume) / abs(rep.volume),
                          "area": rep.area, "area_simplified": r2.area, "area_rel_change": abs(r2.area - rep.area) / abs(rep.area),
                          "closed_oriented_in": int(rep.closed_oriented), "closed_oriented": int(r2.closed_oriented),
                          "nonmanifold_edges": int(r2.nonmanifold_edges), "reps": args.reps, "warmup": args.warmup})
            print(json.dumps(lines[-1]), flush=True)
    if args.output:
        with open(args.output, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
