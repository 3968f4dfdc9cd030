#!/usr/bin/env python3
"""Timing and quality of gsdf_hip_indexed_simplify_adaptive (kernels_simplify_adaptive.h) on the GPU against the uniform
gsdf_hip_indexed_simplify on the same handle.

For each part (`--parts scene:resdiv,...`, per-tree kernels) and each uniform cell of `--cells` x res: the uniform result, then the
adaptive one at MATCHED face count -- finest cell res, `--levels` nested grids, the first tolerance of res / 64, res / 32, ... that
leaves at most as many faces (IndexedHIP.simplify_adaptive_to). Both grids start half a res below the mesh's lattice origin, as
examples/render_ply.py. Timing: after `--warmup` repetitions, `--reps` repetitions in each of which the two routes ALTERNATE (uniform,
adaptive, uniform dry, adaptive dry); the median, minimum and maximum of the stats' own HIP-event times per stage. Quality, side by
side: faces and vertices, the report's edge classes, |volume - input volume|, and the vertex deviation max |d| from the part's
surface before and after gsdf_hip_indexed_project (8 steps, as the example's --project). One JSON line per (part, cell, route).

    python tools/simplify_adaptive_bench.py [--parts npt-flange:400,npt-flange:1600,bolt:200] [--cells 2,4,8] [--levels 8] [--reps 7] [--warmup 2] [-o lines.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="npt-flange:400,npt-flange:1600,bolt:200")
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)

    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    F = np.float32
    lines = []

    def quality(ix, rep_in, sdf, res, max_move):
        r = ix.report()
        moved, ps = ix.project(sdf, res / F(4), res / F(1024), max_move, 8)
        r2 = moved.report()
        return {"n_tris": int(r.n_tris), "n_verts": int(r.n_verts), "closed_oriented": int(r.closed_oriented), "boundary_edges": int(r.boundary_edges),
                "nonmanifold_edges": int(r.nonmanifold_edges), "misoriented_edges": int(r.misoriented_edges), "n_shells": int(r.n_shells),
                "volume_abs_change": abs(r.volume - rep_in.volume), "volume_abs_change_projected": abs(r2.volume - rep_in.volume),
                "area_rel_change": abs(r.area - rep_in.area) / abs(rep_in.area),
                "max_dev_res": ps.max_abs_before / float(res), "max_dev_projected_res": ps.max_abs_after / float(res)}

    for part in args.parts.split(","):
        scene, resdiv = part.split(":")
        resdiv = int(resdiv)
        shape = Builder().Scene(scene)
        sdf = hip.SDF3HIP(shape)
        sdf.specialize()
        res = F(float(shape.Diagonal()) / resdiv)
        mesh = hip.OctreeHIP(sdf, res, payload=hip.PAYLOAD_RECORDS)
        origin = tuple(F(o) - F(0.5) * res for o in mesh.stats.origin[:])
        ix = mesh.weld()
        rep = ix.report()
        dev_in = ix.deviation(sdf, res / F(1024)).max_abs_before / float(res)
        top = res * F(1 << (args.levels - 1))
        for k in [float(x) for x in args.cells.split(",")]:
            cell = F(k) * res
            uni, su = ix.simplify(cell, origin)
            ada, sa, tol = ix.simplify_adaptive_to(int(su.n_tris), res, res / F(64), args.levels, origin)
            runs = {"uniform": [], "adaptive": [], "uniform_dry": [], "adaptive_dry": []}
            for n in range(args.warmup + args.reps):
                got = {"uniform": ix.simplify(cell, origin)[1], "adaptive": ix.simplify_adaptive(res, tol, args.levels, origin)[1],
                       "uniform_dry": ix.simplify(cell, origin, dry=True)[1], "adaptive_dry": ix.simplify_adaptive(res, tol, args.levels, origin, dry=True)[1]}
                if n >= args.warmup:
                    for name, st in got.items():
                        runs[name].append(st)
            base = {"scene": scene, "resdiv": resdiv, "n_tris_in": int(ix.n_tris), "n_verts_in": int(ix.n_verts), "volume_in": rep.volume,
                    "max_dev_in_res": dev_in, "reps": args.reps, "warmup": args.warmup}
            lines.append({**base, "route": "uniform", "cell_res": k, "clusters": int(su.cells), "largest_cluster": int(su.largest_cell),
                          "attempts": int(su.attempts), "table_cells": int(su.table_cells),
                          "ms_cells": spread(s.ms_cells for s in runs["uniform"]), "ms_faces": spread(s.ms_faces for s in runs["uniform"]),
                          "ms_total": spread(s.ms_cells + s.ms_faces for s in runs["uniform"]),
                          "dry_ms_total": spread(s.ms_cells + s.ms_faces for s in runs["uniform_dry"]), **quality(uni, rep, sdf, res, cell)})
            print(json.dumps(lines[-1]), flush=True)
            tot = lambda s: s.ms_cells + s.ms_error + s.ms_faces
            lines.append({**base, "route": "adaptive", "matched_to_cell_res": k, "cell_res": 1.0, "levels": args.levels, "tol_res": float(tol) / float(res),
                          "cells_all_levels": int(sa.cells), "chosen": [int(x) for x in sa.chosen[:args.levels]], "singles": int(sa.singles),
                          "largest_cluster": int(sa.largest_cluster), "max_err_res": sa.max_err / float(res), "attempts": int(sa.attempts),
                          "table_cells": int(sa.table_cells),
                          "ms_cells": spread(s.ms_cells for s in runs["adaptive"]), "ms_error": spread(s.ms_error for s in runs["adaptive"]),
                          "ms_faces": spread(s.ms_faces for s in runs["adaptive"]), "ms_total": spread(tot(s) for s in runs["adaptive"]),
                          "dry_ms_total": spread(tot(s) for s in runs["adaptive_dry"]), **quality(ada, rep, sdf, res, top)})
            print(json.dumps(lines[-1]), flush=True)
            del uni, ada
    if args.output:
        with open(args.output, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
