#!/usr/bin/env python3
"""Mesh one of the reference's example parts on the GPU, weld its marching-cubes vertices there and write an indexed binary PLY:

    python examples/render_ply.py npt-flange --resdiv 400 [--normals] -o npt-flange.ply

The octree mesher leaves the cut-leaf records on the device (payload = records); gsdf_hip_mesh_weld turns them into vertices and
faces by lattice edge -- exact, where a float comparison of the triangle list's corners leaves cracks -- and the file is packed on
the device and arrives in pinned host memory by one DMA (gsdf_hip_indexed_host_ply). Prints V, F, the file's bytes against the
binary STL's of the same mesh, and the weld's device time.

    --report             also print what gsdf_hip_indexed_report says of the mesh (watertight and oriented? shells, volume, area,
                         centre of mass; its device time per stage) and the shell table, and of the mesh that is written its mass
                         properties (gsdf_hip_indexed_mass, on device): mass, centre of mass, the inertia tensor about it, the
                         principal moments and axes; per shell where there are several
    --density RHO        with --report: the density the mass and the inertia are printed for (default 1: volume and unit-density tensor)
    --min-shell-tris N   write the mesh without the shells of fewer than N faces (specks)
    --drop-cavities      ... and without the shells of negative volume (enclosed cavities)
    --simplify K         then merge the vertices of every cell of K x res into one at their mean and drop the faces that collapse
                         (gsdf_hip_indexed_simplify: vertex clustering, on device)
    --max-tris N         ... with the first cell of 2 res, 4 res, 8 res, ... that leaves at most N faces (dry runs find it)
    --adaptive TOL       cluster ADAPTIVELY instead (gsdf_hip_indexed_simplify_adaptive, on device): a vertex goes to the coarsest of
                         --levels nested cells -- the finest of K x res (--simplify K, default 1) -- whose mean stays within TOL x res
                         of the plane of every face touching the cell: flat faces collapse into large cells, thread flanks keep theirs.
                         With --max-tris N: the first tolerance of TOL, 2 TOL, 4 TOL, ... x res that leaves at most N faces
    --levels N           with --adaptive: the number of nested grids (8: cells of up to 128 finest cells)
    --clean              then drop the faces that clustering folded onto each other: of the faces over one set of three vertices at
                         most one stays, opposite pairs cancel (gsdf_hip_indexed_clean, on device; after --simplify / --adaptive,
                         before --project). Prints what it dropped; with --report also the cleaned mesh's report
    --project [ITERS]    then move every vertex onto the part's surface by up to ITERS (8) Newton steps along the field's gradient
                         (gsdf_hip_indexed_project, on device: step res / 4, on the surface within res / 1024, never further than the
                         simplify cell -- or res -- from where it was): clustering pulls the surface inwards on every convex part
    --before-project F   with --project: also write the mesh as it was before the projection to F (the same faces, byte for byte)
    --renderer R         octree (the default: marching cubes, welded by lattice edge) or dualcontour: the reference's sharp-feature
                         mesher straight to an indexed mesh (gsdf_hip_mesh_dualcontour_indexed: one vertex per kept cube, faces in
                         lattice order, the same file byte for byte on every run); every option above works after it
    --chiseled           with --renderer dualcontour: DualContourLeastSquares.Chiseled
    --thickness [THIN]   last, whatever came before: the WALL THICKNESS at every vertex of the mesh that is written -- the distance
                         to the opposite wall along the inward normal, a ray marched through the part's exact field
                         (gsdf_hip_indexed_thickness, on device: from res / 4 inside the surface, normal by central differences of
                         res / 4, on the far wall within res / 1024, at most the bounds' diagonal). Prints min, max, the vertices
                         thinner than THIN (0) and the status table, and writes the thickness as the vertices' `quality` property
                         (+Inf: the ray left the part; NaN: no answer). At a sharp convex edge it is legitimately small
With --simplify / --max-tris, --normals are those of the simplified mesh and --report prints a second report for it; with --project
they are those of the projected mesh, and --report also prints how far the vertices were from the surface before and after, and
the projected mesh's report: its volume is the point of the exercise. The grid starts
HALF A RES BELOW the mesh's lattice origin: two of a marching-cubes vertex's three coordinates lie on lattice planes, in floats whose
last bits depend on which leaf emitted the copy the weld kept (the mesher's order, which varies from run to run); cell faces on
those planes would let these bits decide the cell, cell faces half-way between them make every run cluster alike."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = ["npt-flange", "bolt", "knurled-cylinder", "glyph-plate", "fibonacci-showerhead"]


def print_report(name, ix):
    r = ix.report()
    print(f"{name} report: {'closed and oriented' if r.closed_oriented else 'NOT closed and oriented'}; V {r.n_verts} (used {r.used_verts}) "
          f"E {r.edges} F {r.n_tris}, Euler {r.euler}; degenerate {r.degenerate}, non-finite {r.nonfinite}, boundary {r.boundary_edges}, "
          f"non-manifold {r.nonmanifold_edges}, misoriented {r.misoriented_edges}; {r.n_shells} shells; volume {r.volume:.9g}, area {r.area:.9g}, "
          f"centroid ({r.centroid[0]:.6g}, {r.centroid[1]:.6g}, {r.centroid[2]:.6g}); device {r.ms_edges + r.ms_shells + r.ms_measure:.3f} ms "
          f"(edges {r.ms_edges:.3f}, shells {r.ms_shells:.3f}, measures {r.ms_measure:.3f}; {r.probes} probes of {r.table_cells} cells, {r.attempts} pass)")
    for k, s in enumerate(ix.shells()):
        print(f"  shell {k}: label {s['label']}, V {s['n_verts']} E {s['edges']} F {s['n_tris']}, Euler {s['euler']}, volume {s['volume']:.9g}"
              f"{' (cavity)' if s['volume'] < 0 else ''}, area {s['area']:.9g}, boundary {s['boundary_edges']}, non-manifold {s['nonmanifold_edges']}, "
              f"misoriented {s['misoriented_edges']}")


def print_mass(name, ix, density):
    """Mass properties of the mesh that goes to the file, and of its shells where it has more than one."""
    total, shells = ix.mass(density)

    def line(what, m):
        t, c = m["inertia"], m["centroid"]
        axes = "; ".join("(" + ", ".join(f"{x:.6g}" for x in row) + ")" for row in m["axes"])
        return (f"{what}: mass {m['mass']:.9g} (volume {m['volume']:.9g} at density {density:g}), centre ({c[0]:.6g}, {c[1]:.6g}, {c[2]:.6g}); inertia about it "
                f"xx {t[0, 0]:.9g} yy {t[1, 1]:.9g} zz {t[2, 2]:.9g} xy {t[0, 1]:.9g} xz {t[0, 2]:.9g} yz {t[1, 2]:.9g}; principal moments "
                f"{m['moments'][0]:.9g} {m['moments'][1]:.9g} {m['moments'][2]:.9g} about {axes}")
    print(line(f"{name} mass", total) + f"; device {type(ix).mass_ms():.3f} ms")
    if len(shells) > 1:
        for k, m in enumerate(shells):
            print(line(f"  shell {k} (label {m['label']})", m))


def parse_args(argv=None):
    """The command line, checked: needs no device."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=SCENES)
    ap.add_argument("--resdiv", type=int, default=400, help="resolution = bounding-box diagonal / resdiv (the examples' -resdiv)")
    ap.add_argument("--normals", action="store_true", help="central-difference normals at the vertices (nx ny nz in the file)")
    ap.add_argument("-o", "--output", default=None)
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    ap.add_argument("--report", action="store_true", help="print the mesh's report and its shell table")
    ap.add_argument("--density", type=float, default=1.0, metavar="RHO", help="with --report: the density of the printed mass and inertia")
    ap.add_argument("--min-shell-tris", type=int, default=0, help="drop the shells with fewer faces than this")
    ap.add_argument("--drop-cavities", action="store_true", help="drop the shells of negative volume")
    ap.add_argument("--simplify", type=float, default=0.0, metavar="K", help="cluster the vertices in cells of K x res")
    ap.add_argument("--max-tris", type=int, default=0, metavar="N", help="cluster in cells of 2 res, 4 res, ... until at most N faces are left")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TOL", help="cluster adaptively: a cell's mean stays within TOL x res of its faces' planes")
    ap.add_argument("--levels", type=int, default=8, metavar="N", help="with --adaptive: nested grids, 1 .. 16")
    ap.add_argument("--clean", action="store_true", help="after the clustering: keep at most one face per set of three vertices, cancel opposite pairs")
    ap.add_argument("--project", type=int, nargs="?", const=8, default=None, metavar="ITERS", help="move the vertices onto the surface by up to ITERS (8) Newton steps")
    ap.add_argument("--before-project", default=None, metavar="F", help="with --project: also write the mesh before the projection to F")
    ap.add_argument("--renderer", choices=["octree", "dualcontour"], default="octree", help="the mesher: octree + weld, or dual contouring straight to an indexed mesh")
    ap.add_argument("--chiseled", action="store_true", help="with --renderer dualcontour: the chiseled vertex placement")
    ap.add_argument("--thickness", type=float, nargs="?", const=0.0, default=None, metavar="THIN",
                    help="wall thickness per vertex along the inward normal, written as the quality property; counts the vertices thinner than THIN")
    args = ap.parse_args(argv)
    if args.before_project and args.project is None:
        ap.error("--before-project needs --project")
    if args.chiseled and args.renderer != "dualcontour":
        ap.error("--chiseled needs --renderer dualcontour")
    if args.adaptive is not None and not (args.adaptive >= 0 and 1 <= args.levels <= 16):
        ap.error("--adaptive needs a tolerance >= 0 and --levels 1 .. 16")
    if args.adaptive is not None and args.max_tris > 0 and not args.adaptive > 0:
        ap.error("--adaptive with --max-tris needs a tolerance > 0 to double")
    if args.thickness is not None and not args.thickness >= 0:
        ap.error("--thickness needs a THIN >= 0")
    if not (args.density > 0 and args.density < float("inf")):
        ap.error("--density needs a finite RHO > 0")
    return args


def main(argv=None):
    args = parse_args(argv)

    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    shape = Builder().Scene(args.scene)
    sdf = hip.SDF3HIP(shape)
    if not args.interpreter:
        sdf.specialize()
    res = np.float32(float(shape.Diagonal()) / args.resdiv)
    t0 = time.perf_counter()
    if args.renderer == "dualcontour":
        ix = hip.IndexedHIP.dual_contour(sdf, res, chiseled=args.chiseled)
        t1 = t2 = time.perf_counter()
        mesh_stats = ix.mesh_stats
    else:
        mesh = hip.OctreeHIP(sdf, res, payload=hip.PAYLOAD_RECORDS)
        t1 = time.perf_counter()
        ix = mesh.weld()
        t2 = time.perf_counter()
        mesh_stats = mesh.stats
    adaptive = args.adaptive is not None
    simplify = args.simplify > 0 or args.max_tris > 0 or adaptive
    project = args.project is not None
    if args.normals and not simplify and not project:
        ix.normals(sdf, np.float32(float(res) * 1e-3))
    if args.report:
        print_report(args.scene, ix)
    if args.min_shell_tris > 0 or args.drop_cavities:
        keep = ix.select_shells(args.min_shell_tris, args.drop_cavities)
        whole = ix
        ix = whole.extract(keep)
        print(f"kept {int(keep.sum())} of {len(keep)} shells: V {whole.n_verts} -> {ix.n_verts}, F {whole.n_tris} -> {ix.n_tris} "
              f"(extract {ix.ms_device:.3f} ms device)")
    if simplify:
        whole, origin = ix, tuple(np.float32(o) - np.float32(0.5) * res for o in mesh_stats.origin[:])
        if adaptive:
            fine = np.float32(args.simplify if args.simplify > 0 else 1) * res
            tol = np.float32(args.adaptive) * res
            if args.max_tris > 0:
                ix, ss, tol = whole.simplify_adaptive_to(args.max_tris, fine, tol, args.levels, origin)
            else:
                ix, ss = whole.simplify_adaptive(fine, tol, args.levels, origin)
            cell = fine * np.float32(1 << (args.levels - 1))      # the largest cell: what --project may move a vertex by
            per_level = ", ".join(f"{int(n)} of level {l}" for l, n in enumerate(ss.chosen) if n)
            print(f"simplified adaptively within {float(tol) / float(res):g} res, cells of {float(fine) / float(res):g} res x 1 .. {1 << (args.levels - 1)}: "
                  f"V {whole.n_verts} -> {ix.n_verts}, F {whole.n_tris} -> {ix.n_tris} (clusters: {per_level or 'none'}; {ss.singles} vertices alone, the largest "
                  f"cluster of {ss.largest_cluster} vertices, error at most {ss.max_err / float(res):.4g} res; {ss.cells} cells over all levels, "
                  f"{ss.collapsed} faces collapsed, {ss.degenerate_in} were degenerate; device {ss.ms_cells + ss.ms_error + ss.ms_faces:.3f} ms: cells "
                  f"{ss.ms_cells:.3f}, errors {ss.ms_error:.3f}, faces {ss.ms_faces:.3f}; {ss.probes} probes of {ss.table_cells} cells, {ss.attempts} pass)")
        elif args.max_tris > 0:
            ix, ss, cell = whole.simplify_to(args.max_tris, np.float32(2) * res, origin)
        else:
            cell = np.float32(args.simplify) * res
            ix, ss = whole.simplify(cell, origin)
        if not adaptive:
            print(f"simplified in cells of {float(cell) / float(res):g} res: V {whole.n_verts} -> {ix.n_verts}, F {whole.n_tris} -> {ix.n_tris} "
                  f"({ss.cells} clusters, the largest of {ss.largest_cell} vertices; {ss.collapsed} faces collapsed, {ss.degenerate_in} were degenerate; "
                  f"device {ss.ms_cells + ss.ms_faces:.3f} ms: clusters {ss.ms_cells:.3f}, faces {ss.ms_faces:.3f}; {ss.probes} probes of {ss.table_cells} cells, "
                  f"{ss.attempts} pass)")
        if args.normals and not project:
            ix.normals(sdf, np.float32(float(res) * 1e-3))
        if args.report:
            print_report(args.scene + " simplified", ix)
    if args.clean:
        folded = ix
        ix, cs = folded.clean(merge=False, faces=True)
        print(f"{args.scene} cleaned: V {folded.n_verts} -> {ix.n_verts}, F {folded.n_tris} -> {ix.n_tris} ({cs.opposite_faces} opposite and {cs.duplicate_faces} "
              f"duplicate faces dropped, {cs.degenerate} degenerate; {cs.face_sets} sets, {cs.cancelled_sets} cancelled, the largest of {cs.largest_set} faces; "
              f"device {cs.ms_merge + cs.ms_faces + cs.ms_result:.3f} ms: merge {cs.ms_merge:.3f}, faces {cs.ms_faces:.3f}, result {cs.ms_result:.3f}; "
              f"{cs.face_probes} probes of {cs.face_table_cells} cells, {cs.face_attempts} pass)")
        if args.report:
            print_report(args.scene + " cleaned", ix)
    if project:
        before = ix
        if args.before_project:
            with open(args.before_project, "wb") as f:
                f.write(before.ply_view())
        ix, ps = before.project(sdf, res / np.float32(4), res / np.float32(1024), cell if simplify else res, args.project)
        counts = ", ".join(f"{n.lower()} {ps.count[k]}" for k, n in enumerate(hip.PROJECT_STATUS) if ps.count[k])
        print(f"projected onto the field in up to {args.project} steps: {counts}; {ps.evals} evaluations, at most {ps.steps_max} steps per vertex, "
              f"device {ps.ms_device:.3f} ms")
        if args.normals:
            ix.normals(sdf, np.float32(float(res) * 1e-3))
        if args.report:
            print(f"{args.scene} deviation: max |d| {ps.max_abs_before:.6g} -> {ps.max_abs_after:.6g} ({ps.max_abs_before / float(res):.4g} -> "
                  f"{ps.max_abs_after / float(res):.4g} res); vertices further than res / 1024 from the surface {ps.over_tol_before} -> {ps.over_tol_after} "
                  f"of {ps.n_verts}")
            print_report(args.scene + " projected", ix)
    if args.report:
        print_mass(args.scene, ix, args.density)
    out = args.output or f"{args.scene}.ply"
    data = ix.ply_view()
    if args.thickness is not None:
        from gsdf_amd import ply
        quarter = res / np.float32(4)
        th, status, ts = ix.thickness(sdf, quarter, quarter, np.float32(shape.Diagonal()), res / np.float32(1024), thin=np.float32(args.thickness))
        counts = ", ".join(f"{n.lower()} {ts.count[k]}" for k, n in enumerate(hip.RAY_STATUS) if ts.count[k])
        print(f"{args.scene} thickness: min {ts.t_min:.6g}, max {ts.t_max:.6g} ({ts.t_min / float(res):.4g} .. {ts.t_max / float(res):.4g} res); "
              f"{ts.below} of {ts.n} vertices below {args.thickness:g}; {counts}; {ts.evals} evaluations ({ts.evals / ts.n:.1f} per vertex), "
              f"at most {ts.steps_max} per ray, device {ts.ms_device:.3f} ms")
        v, i, nrm = ply.parse_ply(data)   # the library's own file, and the thickness behind its vertex properties
        data = ply.ply_bytes(v, i, nrm, quality=th)
    with open(out, "wb") as f:
        f.write(data)
    t3 = time.perf_counter()
    st = ix.stats
    stl_bytes = 84 + 50 * ix.n_tris
    print(f"{args.scene} resdiv {args.resdiv}: V {ix.n_verts} F {ix.n_tris}; PLY {len(data)} bytes ({len(data) / ix.n_tris:.1f} per triangle) "
          f"against STL {stl_bytes} bytes; mesh {(t1 - t0) * 1e3:.2f} ms (device {mesh_stats.ms_total:.2f} ms), "
          + (f"of which quads in lattice order {st.ms_keys:.3f} ms and numbering {st.ms_number:.3f} ms device, " if args.renderer == "dualcontour" else
             f"weld {(t2 - t1) * 1e3:.2f} ms (device {ix.ms_device:.3f} ms: keys {st.ms_keys:.3f}, table {st.ms_insert:.3f}, numbering {st.ms_number:.3f}; "
             f"{st.probes} probes of {st.table_cells} cells, {st.attempts} pass), ")
          + f"PLY pack + transfer {st.ms_ply:.3f} ms device; written to {out} in {(t3 - t2) * 1e3:.1f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
