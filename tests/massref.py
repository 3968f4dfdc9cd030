"""A numpy + Python-integer twin of the MASS and SECTION contracts (include/gsdf_hip.h, "indexed meshes: mass properties" and
"contours: section properties"), written from that text: the float64 terms in numpy in the header's order, quantised with np.rint,
summed as Python integers, converted back with one rounding (int / 2**s and float(int) are correctly rounded in Python), the derived
values and the Jacobi iteration in Python floats (IEEE float64, one rounding per operation). Nothing here looks at a device result.
The shells and the exponent are the report's (toporef)."""
import math

import numpy as np

import toporef

TOTAL = 0xffffffff
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]
MASS_DTYPE = np.dtype([("volume", "<f8"), ("first", "<f8", (3,)), ("second", "<f8", (6,)), ("centroid", "<f8", (3,)), ("inertia", "<f8", (6,)),
                       ("exponent", "<i4"), ("label", "<u4")])
SECTION_DTYPE = np.dtype([("area", "<f8"), ("first", "<f8", (2,)), ("second", "<f8", (3,)), ("centroid", "<f8", (2,)), ("central", "<f8", (3,)),
                          ("n_verts", "<u4"), ("layer_or_n_loops", "<u4")])
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # xx yy zz xy xz yz


def _value(t, shift):
    """The integer t times 2^-shift as float64, one rounding (the result is never subnormal in either contract)."""
    return float(t / (1 << shift)) if shift >= 0 else float(t << -shift)


def _quantise(term, shift):
    """Python integers: round(term * 2^shift), ties to even."""
    with np.errstate(all="ignore"):
        return [int(x) for x in np.rint(term * math.ldexp(1.0, shift)).astype(np.int64)]


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def face_terms(a, b, c):
    """The ten float64 terms of faces with corners a, b, c (n, 3) float32: volume, first x y z, second xx yy zz xy xz yz."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        mx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
        my = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
        mz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
        det = (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz
        s = (a + b) + c
        out = [det / 6.0] + [(det * s[:, k]) / 24.0 for k in range(3)]
        for i, j in PAIRS:
            out.append((det * ((((a[:, i] * a[:, j]) + (b[:, i] * b[:, j])) + (c[:, i] * c[:, j])) + (s[:, i] * s[:, j]))) / 120.0)
    return out


def mesh_ints(verts, idx):
    """(e, labels (n_shells,), ints: n_shells lists of the ten integers) over the finite non-degenerate faces of every shell."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    an = toporef.analyse(v, i)
    sof = an["shell_of_face"].astype(np.int64)
    n_shells = len(an["shells"])
    e = toporef.exponent_of(v)
    live = sof != toporef.NONE
    live &= np.isfinite(v[i.reshape(-1)]).reshape(-1, 9).all(axis=1)
    f, fs = i[live], sof[live]
    shifts = [62 - 3 * e] + [62 - 4 * e] * 3 + [62 - 5 * e] * 6
    ints = [[0] * 10 for _ in range(n_shells)]
    for k, t in enumerate(face_terms(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])):
        for shell, q in zip(fs, _quantise(t, shifts[k])):
            ints[shell][k] += q
    return e, an["shells"]["label"].astype(np.uint32), ints


def mass_record(ints, e, label):
    """The record of ten integers: the header's conversions and derived values, one float64 operation each."""
    r = np.zeros(1, MASS_DTYPE)[0]
    vol = _value(ints[0], 62 - 3 * e)
    first = [_value(ints[1 + k], 62 - 4 * e) for k in range(3)]
    second = [_value(ints[4 + k], 62 - 5 * e) for k in range(6)]
    r["volume"], r["first"], r["second"], r["exponent"], r["label"] = vol, first, second, e, label
    if vol == 0.0:
        r["centroid"], r["inertia"] = QNAN, QNAN
        return r
    r["centroid"] = [first[k] / vol for k in range(3)]
    c = [second[k] - ((first[i] * first[j]) / vol) for k, (i, j) in enumerate(PAIRS)]
    r["inertia"] = [c[1] + c[2], c[0] + c[2], c[0] + c[1], -c[3], -c[4], -c[5]]
    return r


def mesh_mass(verts, idx):
    """(total record, shells' records (MASS_DTYPE array), the shells' integers)."""
    e, labels, ints = mesh_ints(verts, idx)
    shells = np.zeros(len(ints), MASS_DTYPE)
    for k, row in enumerate(ints):
        shells[k] = mass_record(row, e, labels[k])
    tot = [sum(row[k] for row in ints) for k in range(10)]
    return mass_record(tot, e, TOTAL), shells, ints


def principal(inertia):
    """gsdf_hip_inertia_principal's sequence in Python floats: (moments (3,), axes (3, 3) float64)."""
    m = [float(x) for x in inertia]
    assert all(math.isfinite(x) for x in m)
    a = [[m[0], m[3], m[4]], [m[3], m[1], m[5]], [m[4], m[5], m[2]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(32):
        if a[0][1] == 0.0 and a[0][2] == 0.0 and a[1][2] == 0.0:
            break
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            g = a[p][q]
            if g == 0.0:
                continue
            if abs(a[p][p]) + abs(g) == abs(a[p][p]) and abs(a[q][q]) + abs(g) == abs(a[q][q]):
                a[p][q] = a[q][p] = 0.0
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * g)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt((theta * theta) + 1.0))
            c = 1.0 / math.sqrt((t * t) + 1.0)
            s = t * c
            h = t * g
            a[p][p] = a[p][p] - h
            a[q][q] = a[q][q] + h
            a[p][q] = a[q][p] = 0.0
            x, y = a[r][p], a[r][q]
            a[r][p] = a[p][r] = (c * x) - (s * y)
            a[r][q] = a[q][r] = (s * x) + (c * y)
            for i in range(3):
                x, y = v[i][p], v[i][q]
                v[i][p] = (c * x) - (s * y)
                v[i][q] = (s * x) + (c * y)
    order = [0, 1, 2]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if a[order[i]][order[i]] > a[order[j]][order[j]]:
            order[i], order[j] = order[j], order[i]
    moments = [a[k][k] for k in order]
    axes = []
    for k in order[:2]:
        x = [v[i][k] for i in range(3)]
        big = 0
        for i in (1, 2):
            if abs(x[i]) > abs(x[big]):
                big = i
        if x[big] < 0.0:
            x = [-t for t in x]
        axes.append(x)
    x, y = axes
    axes.append([(x[1] * y[2]) - (x[2] * y[1]), (x[2] * y[0]) - (x[0] * y[2]), (x[0] * y[1]) - (x[1] * y[0])])
    return np.array(moments, np.float64), np.array(axes, np.float64)


# ---- loops ----------------------------------------------------------------------------------------------------------------------------
def loop_exponent(xy):
    bits = np.ascontiguousarray(xy, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    return max(int(bits.max()) >> 23 if bits.size else 0, 1) - 126


def loop_ints(xy, loop_start):
    """(e, ints: per loop the six integers twice-the-area (the measures' sum), first x y, second xx yy xy)."""
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    ls = np.asarray(loop_start).astype(np.int64)
    e = loop_exponent(p)
    shifts = [61 - 2 * e, 62 - 3 * e, 62 - 3 * e, 62 - 4 * e, 62 - 4 * e, 62 - 4 * e]
    ints = []
    for q in range(len(ls) - 1):
        a = p[ls[q]:ls[q + 1]].astype(np.float64)
        b = np.roll(a, -1, axis=0)
        x0, y0, x1, y1 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
        with np.errstate(all="ignore"):
            cross = x0 * y1 - x1 * y0
            terms = [cross,
                     (cross * (x0 + x1)) / 6.0,
                     (cross * (y0 + y1)) / 6.0,
                     (cross * (((x0 * x0) + (x0 * x1)) + (x1 * x1))) / 12.0,
                     (cross * (((y0 * y0) + (y0 * y1)) + (y1 * y1))) / 12.0,
                     (cross * ((((x0 * y1) + (x1 * y0)) + 2.0 * (x0 * y0)) + 2.0 * (x1 * y1))) / 24.0]
        ints.append([sum(_quantise(t, s)) for t, s in zip(terms, shifts)])
    return e, ints


def section_record(ints, e, n_verts, layer_or_n_loops):
    r = np.zeros(1, SECTION_DTYPE)[0]
    area = _value(ints[0], 62 - 2 * e)
    first = [_value(ints[1 + k], 62 - 3 * e) for k in range(2)]
    second = [_value(ints[3 + k], 62 - 4 * e) for k in range(3)]
    r["area"], r["first"], r["second"], r["n_verts"], r["layer_or_n_loops"] = area, first, second, n_verts, layer_or_n_loops
    if area == 0.0:
        r["centroid"], r["central"] = QNAN, QNAN
        return r
    r["centroid"] = [first[k] / area for k in range(2)]
    r["central"] = [second[k] - ((first[i] * first[j]) / area) for k, (i, j) in enumerate(((0, 0), (1, 1), (0, 1)))]
    return r


def sections(xy, loop_start, loop_layer=None, n_layers=1):
    """(loops' records, layers' records (SECTION_DTYPE arrays), the loops' integers)."""
    ls = np.asarray(loop_start).astype(np.int64)
    n_loops = len(ls) - 1
    layer = np.zeros(n_loops, np.int64) if loop_layer is None else np.asarray(loop_layer).astype(np.int64)
    e, ints = loop_ints(xy, ls)
    loops, layers = np.zeros(n_loops, SECTION_DTYPE), np.zeros(n_layers, SECTION_DTYPE)
    for q in range(n_loops):
        loops[q] = section_record(ints[q], e, ls[q + 1] - ls[q], layer[q])
    for l in range(n_layers):
        mine = [q for q in range(n_loops) if layer[q] == l]
        tot = [sum(ints[q][k] for q in mine) for k in range(6)]
        layers[l] = section_record(tot, e, sum(int(ls[q + 1] - ls[q]) for q in mine), len(mine))
    return loops, layers, ints


# ---- hand shapes with closed forms ------------------------------------------------------------------------------------------------------
def box(lo, hi, inward=False):
    """An axis-aligned box lo (3,) .. hi (3,) as 8 vertices and 12 outward (or inward) triangles."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[x][0], (lo, hi)[y][1], (lo, hi)[z][2]] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    i = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return v, (i[:, ::-1].copy() if inward else i)


def box_moments(lo, hi):
    """Closed forms of a box: volume, first (3,), second (6,) about the origin, as exact fractions evaluated in float64."""
    from fractions import Fraction as Fr
    lo, hi = [Fr(float(x)) for x in lo], [Fr(float(x)) for x in hi]
    d = [h - l for l, h in zip(lo, hi)]
    m1 = [(h * h - l * l) / 2 for l, h in zip(lo, hi)]   # integral of x over [l, h]
    m2 = [(h ** 3 - l ** 3) / 3 for l, h in zip(lo, hi)]
    vol = d[0] * d[1] * d[2]
    first = [m1[k] * vol / d[k] for k in range(3)]
    second = [m2[i] * vol / d[i] if i == j else m1[i] * m1[j] * vol / (d[i] * d[j]) for i, j in PAIRS]
    return float(vol), [float(x) for x in first], [float(x) for x in second]


def sphere(n_lat, n_lon, r=1.0, centre=(0.0, 0.0, 0.0)):
    """A closed, outward-oriented latitude / longitude sphere: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) faces."""
    v = [[0.0, 0.0, r]]
    for a in range(1, n_lat):
        th = math.pi * a / n_lat
        for b in range(n_lon):
            ph = 2 * math.pi * b / n_lon
            v.append([r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)])
    v.append([0.0, 0.0, -r])
    south = len(v) - 1
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon
    f = []
    for b in range(n_lon):
        f.append((0, ring(1, b), ring(1, b + 1)))
        f.append((south, ring(n_lat - 1, b + 1), ring(n_lat - 1, b)))
        for a in range(1, n_lat - 1):
            f.append((ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)))
            f.append((ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)))
    return (np.array(v, np.float64) + np.asarray(centre, np.float64)).astype(np.float32), np.array(f, np.uint32)
