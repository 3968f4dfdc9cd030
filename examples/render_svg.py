#!/usr/bin/env python3
"""Vector outlines traced on the GPU, written as SVG: the curve a laser cutter or plotter takes for a 2-D part, and the contours a
slicer wants of a 3-D part at each layer height:

    python examples/render_svg.py text -o text.svg                             # the 2-D scenes of render_png.py: image, text, thread
    python examples/render_svg.py npt-flange --slice 5 -o flange.svg           # one contour of a 3-D scene (npt-flange, bolt) at z = 5
    python examples/render_svg.py bolt --layer-height 2 --report -o bolt.svg   # every layer of thickness 2, with a report
    python examples/render_svg.py text --simplify 0.125 --report -o text.svg   # vertices within res / 8 of a chord dropped on the GPU
    python examples/render_svg.py bolt --layer-height 2 --hatch 4 --report -o bolt.svg   # hatch lines 4 res apart, 45 / 135 degrees by layer
    python examples/render_svg.py bolt --layer-height 2 --hatch 4 --skin 1 1 --report    # the hatch classed as inner, bottom, top skin
    python examples/render_svg.py bolt --layer-height 2 --walls 3 --wall-width 4 --hatch 4 --report   # three walls 4 res wide, the fill inside them

The lattice spacing is the diagonal of the part's bounds / --resdiv (default 400), or --res. Every layer is one even-odd <path>:
outer boundaries counter-clockwise, holes clockwise. --report prints loops, vertices, outer and hole counts and the area of every
layer, and the device time of the two stages (evaluation, tracing). --simplify TOL drops the vertices that lie within TOL x res of a
dyadic chord of their loop (gsdf_hip_contour_simplify; --levels, --passes as there), --max-verts N doubles that tolerance until at
most N vertices are left; the report then adds the vertices before and after, the largest deviation and the layers' areas and lengths
summed on the device. The report ends with the section properties of every layer that is written (gsdf_hip_contour_sections, on
device): the centroid and the second moments of area about it. --hatch SPACING fills every layer with the segments of parallel lines
SPACING x res apart that lie inside the material (gsdf_hip_contour_hatch, on device; on the simplified loops when --simplify is
given), at the angles of --hatch-angle in turn by layer; they are drawn as <line> elements, and the report adds the segments and the
hatch length of every layer, the most crossings on one line and the device time. --skin BELOW ABOVE (with --hatch) cuts every hatch
line against the loops of the BELOW layers under and the ABOVE layers over its layer (gsdf_hip_contour_hatch_skin, on device) and
draws the pieces in one stroke per class: inner, bottom skin, top skin, both; the report then gives length x spacing of every class,
per layer and in total (an estimate of its area), and the layers above the first BELOW that still have bottom skin: the overhangs.
--walls N --wall-width W draws N perimeters inside every layer's outline, at the in-plane distances (i + 0.5) W x res (the middle of
bead i; gsdf_hip_contour_offset, on device, from the loops themselves), as unfilled paths of their own class; --hatch and --skin then
fill the loops of a second, single-inset offset at N W x res, the inner edge of the wall stack, instead of the raw outline, and the
report adds the walls' lengths per layer (gsdf_hip_contour_measures on the offset handle) and the device time of the distance field
and of the tracing. The SVG is written with the standard library only."""
import argparse
import importlib.util
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES_2D = ("image", "text", "thread")
SCENES_3D = ("npt-flange", "bolt")


def scene(name):
    """The 2-D scenes are render_png.py's; the 3-D ones the scaffold's benchmark scenes."""
    if name in SCENES_2D:
        spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.scene(name)
    from scaffold.builder import Builder
    return Builder().Scene(name)


def spacing(bb, is3d, resdiv):
    """The default lattice spacing: the diagonal of the bounds (xy for a 2-D part) / resdiv, float32."""
    import numpy as np
    return np.float32(math.sqrt(sum(float(bb[a + 3] - bb[a]) ** 2 for a in ((0, 1, 2) if is3d else (0, 1)))) / resdiv)


def trace(hip, sdf, res, z=None):
    """A ContourHIP of `sdf`: its outline (2-D) or its slices at the heights z (3-D)."""
    return hip.ContourHIP.outline(sdf, res) if sdf.is2d else hip.ContourHIP.slices(sdf, res, z)


def report(c, z=None):
    import numpy as np
    st = c.stats
    areas = c.areas()
    lines = [f"lattice {st.nx} x {st.ny} x {st.n_layers} layers = {st.evals} evaluations; {st.n_loops} loops, {st.n_verts} vertices, "
             f"{st.saddle_cells} saddle cells, {st.nonfinite_nodes} non-finite nodes, {st.border_inside} forced outside; {st.rank_rounds} ranking rounds",
             f"device time {st.ms_device:.3f} ms = evaluation {st.ms_eval:.3f} + tracing {st.ms_trace:.3f} "
             f"({st.evals / max(st.ms_eval, 1e-9) / 1e6:.1f} G evaluations/s in the evaluation stage)"]
    for k in range(c.n_layers):
        a = areas[c.loop_layer == k]
        n = int(sum(c.loop_start[q + 1] - c.loop_start[q] for q in range(c.n_loops) if c.loop_layer[q] == k))
        at = "" if z is None else f" z = {float(np.float32(z[k])):.6g}:"
        lines.append(f"layer {k}:{at} {len(a)} loops ({int((a > 0).sum())} outer, {int((a < 0).sum())} holes), {n} vertices, area {a.sum():.6g}")
    return "\n".join(lines)


def simplify_report(before, c, st, tol):
    """What --simplify did, and the simplified layers' measures from the device."""
    lines = [f"simplified at tol {float(tol):.6g}: {before} -> {c.n_verts} vertices in {c.n_loops} loops ({st.loops_changed} loops changed), max_dev {st.max_dev:.6g}, "
             f"largest span level {st.max_level}, device time {st.ms_device:.3f} ms"]
    _, layers = c.measures()
    for k, m in enumerate(layers):
        lines.append(f"layer {k} on the device: {m['n_loops']} loops, {m['n_verts']} vertices, area {m['area']:.9g}, length {m['length']:.9g} "
                     f"(measures: {type(c).measures_ms():.3f} ms)")
    return "\n".join(lines)


def section_report(c):
    """Centroid and central second moments of area of the written layers, from the device."""
    _, layers = c.sections()
    return "\n".join(f"layer {k} section: area {s['area']:.9g}, centroid ({s['centroid'][0]:.6g}, {s['centroid'][1]:.6g}), second moments about it "
                     f"xx {s['central'][0]:.9g} yy {s['central'][1]:.9g} xy {s['central'][2]:.9g} (sections: {type(c).sections_ms():.3f} ms)"
                     for k, s in enumerate(layers))


def hatch_report(h, c):
    """What --hatch made: per layer the segments and their length, then the cost."""
    st = h.stats
    lines = [f"layer {k} hatch: {int(m['n_segments'])} segments, length {m['length']:.9g}, lines {int(m['k_min'])} .. {int(m['k_max'])}" for k, m in enumerate(h.layers)]
    lines.append(f"hatch: {st.n_segments} segments on {st.n_lines} lines, length {st.length:.9g}, {st.zero_length} of zero length, max_line_crossings "
                 f"{st.max_line_crossings}, device time {st.ms_device:.3f} ms (rank pass {type(c).hatch_rank_ms():.3f} ms)")
    return "\n".join(lines)


def skin_report(h, c, spacing, below):
    """What --skin made: per layer and in total the area estimate length x spacing of every class, the overhanging layers, the cost."""
    from gsdf_amd.hip import SKIN_CLASSES
    st = h.stats
    by_class = lambda length, n: ", ".join(f"{name} {float(length[q]) * spacing:.9g} ({int(n[q])})" for q, name in enumerate(SKIN_CLASSES))  # noqa: E731
    lines = [f"layer {k} skin area (pieces): {by_class(m['length'], m['n_segments'])}" for k, m in enumerate(h.skin_layers)]
    lines.append(f"skin area (pieces) in all: {by_class(st.length, st.n_class)}")
    over = [f"layer {k} {float(m['length'][1] + m['length'][3]) * spacing:.9g}" for k, m in enumerate(h.skin_layers)
            if k >= below and (m["n_segments"][1] or m["n_segments"][3])]
    lines.append(f"overhangs (bottom skin above layer {below - 1}): " + (", ".join(over) or "none"))
    lines.append(f"skin: window {st.below} below, {st.above} above; {st.n_segments} pieces on {st.n_lines} lines from {st.n_crossings} crossings ({st.n_own_crossings} own), "
                 f"{st.zero_length} of zero length, max_line_crossings {st.max_line_crossings}, device time {st.ms_device:.3f} ms (rank pass {type(c).skin_rank_ms():.3f} ms)")
    return "\n".join(lines)


def walls_report(walls, n, width, fill):
    """What --walls made: per layer the length of every wall (measures on the offset handle), then the cost of the two offsets."""
    _, layers = walls.measures()
    lines = []
    for k in range(walls.n_layers // n):
        each = [float(layers[k * n + i]["length"]) for i in range(n)]
        lines.append(f"layer {k} walls: length " + " + ".join(f"{v:.9g}" for v in each) + f" = {sum(each):.9g} ({sum(int(layers[k * n + i]['n_loops']) for i in range(n))} loops)")
    for name, c in (("walls", walls), ("fill boundary", fill)):
        st = c.offset_stats
        lines.append(f"{name}: {st.n_insets} inset(s) of width {width:.6g} on a lattice {st.nx} x {st.ny} x {st.n_layers_in} layers, band {st.band:.6g}: {st.n_loops} loops, "
                     f"{st.n_verts} vertices, {st.inside_nodes} nodes inside, {st.band_nodes} in the band, {st.saddle_cells} saddle cells; device time {st.ms_device:.6g} ms = "
                     f"distance field {st.ms_field:.6g} + tracing {st.ms_trace:.6g}")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=SCENES_2D + SCENES_3D)
    ap.add_argument("--res", type=float, default=None, help="lattice spacing (default: diagonal of the bounds / --resdiv)")
    ap.add_argument("--resdiv", type=float, default=400.0)
    ap.add_argument("--slice", type=float, default=None, metavar="Z", help="3-D scenes: one contour at this height")
    ap.add_argument("--layer-height", type=float, default=None, metavar="H", help="3-D scenes: a contour at the middle of every layer of this thickness")
    ap.add_argument("--simplify", type=float, default=None, metavar="TOL", help="drop vertices within TOL x res of a dyadic chord of their loop")
    ap.add_argument("--levels", type=int, default=8, help="--simplify: dyadic levels, 1 .. 16")
    ap.add_argument("--passes", type=int, default=1, help="--simplify: passes, 1 .. 8 (the deviations add)")
    ap.add_argument("--max-verts", type=int, default=None, metavar="N", help="--simplify: double the tolerance until at most N vertices are left")
    ap.add_argument("--hatch", type=float, default=None, metavar="SPACING", help="fill the layers with parallel lines SPACING x res apart")
    ap.add_argument("--hatch-angle", type=float, nargs="+", default=[45.0, 135.0], metavar="DEG", help="--hatch: the lines' angles, in turn by layer (1 .. 4)")
    ap.add_argument("--skin", type=int, nargs=2, default=None, metavar=("BELOW", "ABOVE"), help="--hatch: class the hatch by the layers under and over (0 .. 8 each)")
    ap.add_argument("--walls", type=int, default=None, metavar="N", help="N perimeters inside the outline (1 .. 8), the fill inside them")
    ap.add_argument("--wall-width", type=float, default=None, metavar="W", help="--walls: the width of one wall, W x res")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)
    if args.skin is not None and args.hatch is None:
        ap.error("--skin classes the hatch: it goes with --hatch SPACING")
    if (args.walls is None) != (args.wall_width is None):
        ap.error("--walls N and --wall-width W go together")
    if args.walls is not None and not (1 <= args.walls <= 8 and args.wall_width > 0):
        ap.error("--walls takes 1 .. 8 walls of a positive width")

    import numpy as np
    from gsdf_amd import hip, svg

    is3d = args.scene in SCENES_3D
    if is3d == (args.slice is None and args.layer_height is None) or (args.slice is not None and args.layer_height is not None):
        ap.error("a 3-D scene takes --slice Z or --layer-height H; a 2-D scene takes neither")
    hip.init(0)
    t0 = time.perf_counter()
    s = scene(args.scene)
    sdf = (hip.SDF3HIP if is3d else hip.SDF2HIP)(s)
    if not args.interpreter:
        sdf.specialize()
    bb = sdf.Bounds()
    res = np.float32(args.res) if args.res is not None else spacing(bb, is3d, args.resdiv)
    z = None
    if is3d:
        z = np.array([args.slice], np.float32) if args.slice is not None else hip.layer_heights(bb, args.layer_height)
        if len(z) == 0:
            ap.error("no layer of that thickness has its middle inside the part")
    t1 = time.perf_counter()
    c = trace(hip, sdf, res, z)
    t2 = time.perf_counter()
    traced, simplified = c, None
    if args.simplify is not None:
        tol = np.float32(np.float32(args.simplify) * res)
        if args.max_verts is not None:
            c, st, tol = traced.simplify_to(args.max_verts, tol, args.levels, args.passes)
        else:
            c, st = traced.simplify(tol, args.levels, args.passes)
        simplified = (st, tol)
    elif args.max_verts is not None:
        ap.error("--max-verts goes with --simplify TOL, the tolerance the doubling starts from")
    out = args.output or f"{args.scene}.svg"
    hatch = hatch_class = walls = None
    fill = c  # the loops the hatch fills: the outline, or with --walls the inner edge of the wall stack
    if args.walls is not None:
        wall_width = np.float32(np.float32(args.wall_width) * res)
        walls = c.offset(res, [np.float32(np.float32(i + 0.5) * wall_width) for i in range(args.walls)])
        fill = c.offset(res, [np.float32(np.float32(args.walls) * wall_width)])
    if args.hatch is not None:
        hatch_spacing = np.float32(np.float32(args.hatch) * res)
        hatch = fill.hatch(hatch_spacing, args.hatch_angle) if args.skin is None else fill.skin(hatch_spacing, args.hatch_angle, *args.skin)
        if args.skin is not None:
            hatch_class = [hatch.cls[hatch.layer_start[k]:hatch.layer_start[k + 1]] for k in range(hatch.n_layers)]
    svg.write_svg(out, [c.loops(k) for k in range(c.n_layers)], z=z, hatch=None if hatch is None else [hatch.segments(k) for k in range(hatch.n_layers)],
                  hatch_class=hatch_class, walls=None if walls is None else [[walls.loops(k * args.walls + i) for i in range(args.walls)] for k in range(c.n_layers)])
    print(f"{args.scene} res {float(res):.6g}: setup {t1 - t0:.2f} s, contours {(t2 - t1) * 1e3:.1f} ms (the first call includes the kernels' build); "
          f"{c.n_loops} loops, {c.n_verts} vertices in {c.n_layers} layer(s); written to {out}")
    if args.report:
        print(report(traced, z))
        if simplified:
            print(simplify_report(traced.n_verts, c, *simplified))
        print(section_report(c))
        if walls is not None:
            print(walls_report(walls, args.walls, float(wall_width), fill))
        if hatch is not None:
            print(hatch_report(hatch, c) if args.skin is None else skin_report(hatch, c, float(hatch_spacing), args.skin[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
