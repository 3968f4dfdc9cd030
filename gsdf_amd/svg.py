"""SVG outlines with the standard library only (struct, re): the loops of a ContourHIP as one even-odd <path> per layer, their hatch
segments (a HatchHIP's) as <line> elements in a group of their own (a skin hatch's in one stroke per class), the walls of a
ContourHIP.offset as unfilled paths of their own class, and the readers. Coordinates are written as the shortest decimal that reads back as the same float32, so write followed by read is bit-exact;
the y axis points up in the part and down in SVG, and is turned by one transform around the paths, not by changing coordinates."""
import re
import struct

import numpy as np


def fmt(v):
    """The shortest decimal (%.{p}g, p = 1 .. 9) that rounds back to the float32 `v`, to the bit (negative zero, subnormals)."""
    v = float(v)
    want = struct.pack("<f", v)
    if want in (b"\x00\x00\x80\x7f", b"\x00\x00\x80\xff") or v != v:
        raise ValueError("a coordinate is not finite")
    for p in range(1, 10):
        s = "%.*g" % (p, v)
        try:
            if struct.pack("<f", float(s)) == want:
                return s
        except OverflowError:  # (a shorter decimal of the largest floats rounds past them)
            pass
    raise AssertionError("nine digits always identify a float32")


SKIN_STROKES = ("#a04020", "#2060c0", "#20a040", "#a020a0")  # by class: inner (the plain hatch's stroke), bottom, top, both
WALL_STROKE = "#206040"


def _path_data(loops):
    d = []
    for l in loops:
        a = np.asarray(l, np.float32).reshape(-1, 2)
        if len(a) == 0:
            continue
        d.append("M " + " L ".join("%s %s" % (fmt(x), fmt(y)) for x, y in a) + " Z")
    return " ".join(d)


def write_svg(path, layers, z=None, stroke_width=None, hatch=None, hatch_class=None, walls=None):
    """layers: a list (one entry per layer) of lists of loops, each loop (n, 2) float32 in order of travel. One
    <path fill-rule="evenodd"> per layer (an empty layer: an empty path), each loop `M x y L x y ... Z`. z (optional): the layers'
    heights, kept as data-z. hatch (optional): per layer an (n, 4) float32 array of segments x0 y0 x1 y1 (HatchHIP.segments(k)),
    drawn as <line> elements in one <g id="hatchK"> per layer after the paths: never as <path>, which read_svg takes for a layer.
    hatch_class (optional, with hatch): per layer the n classes 0 .. 3 of its segments (HatchHIP.cls of a skin hatch); every line
    then carries data-class and its class's stroke (SKIN_STROKES). Without it the file is what it was before classes existed.
    walls (optional): per layer a list (one entry per wall, outermost first) of lists of loops (the layers of a ContourHIP.offset):
    one unfilled <path class="wall" id="wallK_I"> each, in one <g id="wallsK"> per layer between the layers' paths and the hatch;
    read_svg leaves them out and read_svg_walls returns them. Without it the file is what it was before walls existed."""
    lo, hi = [None, None], [None, None]
    for loops in layers:
        for l in loops:
            a = np.asarray(l, np.float32).reshape(-1, 2)
            if len(a):
                for k in (0, 1):
                    mn, mx = float(a[:, k].min()), float(a[:, k].max())
                    lo[k] = mn if lo[k] is None else min(lo[k], mn)
                    hi[k] = mx if hi[k] is None else max(hi[k], mx)
    if lo[0] is None:
        lo, hi = [0.0, 0.0], [1.0, 1.0]
    w, h = max(hi[0] - lo[0], 1e-30), max(hi[1] - lo[1], 1e-30)
    pad = 0.02 * max(w, h)
    sw = stroke_width if stroke_width is not None else 0.002 * max(w, h)
    out = ['<?xml version="1.0" encoding="UTF-8"?>\n',
           '<svg xmlns="http://www.w3.org/2000/svg" viewBox="%.9g %.9g %.9g %.9g">\n' % (lo[0] - pad, -(hi[1] + pad), w + 2 * pad, h + 2 * pad),
           '<g transform="scale(1,-1)" fill="#c8d4e4" stroke="#203040" stroke-width="%.9g">\n' % sw]
    for k, loops in enumerate(layers):
        zattr = "" if z is None else ' data-z="%s"' % fmt(np.float32(z[k]))
        out.append('<path id="layer%d"%s fill-rule="evenodd" d="%s"/>\n' % (k, zattr, _path_data(loops)))
    if walls is not None:
        out.append('<g id="walls" fill="none" stroke="%s" stroke-width="%.9g">\n' % (WALL_STROKE, 0.75 * sw))
        for k, per_wall in enumerate(walls):
            out.append('<g id="walls%d">\n' % k)
            for i, loops in enumerate(per_wall):
                out.append('<path class="wall" id="wall%d_%d" fill-rule="evenodd" d="%s"/>\n' % (k, i, _path_data(loops)))
            out.append("</g>\n")
        out.append("</g>\n")
    if hatch is not None:
        out.append('<g id="hatch" fill="none" stroke="#a04020" stroke-width="%.9g">\n' % (0.5 * sw))
        for k, segs in enumerate(hatch):
            out.append('<g id="hatch%d">\n' % k)
            segs = np.asarray(segs, np.float32).reshape(-1, 4)
            cls = None if hatch_class is None else np.asarray(hatch_class[k], np.uint8).reshape(-1)
            if cls is not None and (len(cls) != len(segs) or (cls > 3).any()):
                raise ValueError("hatch_class must give every segment of a layer a class 0 .. 3")
            for i, (x0, y0, x1, y1) in enumerate(segs):
                extra = "" if cls is None else ' data-class="%d" stroke="%s"' % (cls[i], SKIN_STROKES[cls[i]])
                out.append('<line x1="%s" y1="%s" x2="%s" y2="%s"%s/>\n' % (fmt(x0), fmt(y0), fmt(x1), fmt(y1), extra))
            out.append("</g>\n")
        out.append("</g>\n")
    out.append("</g>\n</svg>\n")
    with open(path, "w", encoding="utf-8") as f:
        f.write("".join(out))


_PATH = re.compile(r'<path\b[^>]*?\bd="([^"]*)"[^>]*/>')
_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_LOOP = re.compile(r"M\s*((?:%s[\s,]*|L\s*)+)Z" % _NUM)


_LINE = re.compile(r'<line x1="(%s)" y1="(%s)" x2="(%s)" y2="(%s)"(?: data-class="([0-3])" stroke="#[0-9a-f]{6}")?/>' % ((_NUM,) * 4))


def read_svg_hatch(path):
    """The hatch segments of a file written by write_svg(..., hatch=...): per <g id="hatchK"> an (n, 4) float32 array."""
    text = open(path, encoding="utf-8").read()
    return [np.array([[float(v) for v in m.groups()[:4]] for m in _LINE.finditer(g)], np.float64).astype(np.float32).reshape(-1, 4)
            for g in re.findall(r'<g id="hatch\d+">(.*?)</g>', text, flags=re.S)]


def read_svg_hatch_class(path):
    """The classes of the hatch segments of a file written by write_svg(..., hatch_class=...): per <g id="hatchK"> n uint8; a
    file without classes raises ValueError."""
    text = open(path, encoding="utf-8").read()
    out = []
    for g in re.findall(r'<g id="hatch\d+">(.*?)</g>', text, flags=re.S):
        cls = [m.group(5) for m in _LINE.finditer(g)]
        if None in cls:
            raise ValueError("a hatch segment without a class")
        out.append(np.array([int(c) for c in cls], np.uint8))
    return out


def _loops_of(d):
    loops = []
    for lm in _LOOP.finditer(d):
        vals = [float(s) for s in re.findall(_NUM, lm.group(1))]
        if len(vals) % 2:
            raise ValueError("odd number of coordinates in a loop")
        loops.append(np.array(vals, np.float64).astype(np.float32).reshape(-1, 2))
    return loops


def read_svg(path):
    """The loops of a file written by write_svg: a list per layer (per <path> that is no wall) of (n, 2) float32 arrays."""
    text = open(path, encoding="utf-8").read()
    return [_loops_of(m.group(1)) for m in _PATH.finditer(text) if ' class="wall"' not in m.group(0)]


def read_svg_walls(path):
    """The walls of a file written by write_svg(..., walls=...): per <g id="wallsK"> a list (one entry per wall) of lists of (n, 2)
    float32 loops."""
    text = open(path, encoding="utf-8").read()
    return [[_loops_of(m.group(1)) for m in _PATH.finditer(g)] for g in re.findall(r'<g id="walls\d+">(.*?)</g>', text, flags=re.S)]
