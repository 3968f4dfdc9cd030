"""The CPU twins of the loop-stack family (contoursimpref, massref, hatchref, skinref, offsetref) on the ground of tests/loop_corpus.py:
repeated vertices, points, flattened loops, bow-ties, repeated loops, vertices on hatch lines and lattice nodes, 300 layers, counts that
are exact multiples. No GPU. Every twin must run on every case; a census states what the generator's seeds reach, so that an edit of it
cannot quietly make the corpus tame; closed forms hold the twins where one exists. The device is held to the twins, to the byte, in
tests/test_gpu_loop_corpus.py."""
import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
import loop_corpus as LC
import offsetref as O

F = np.float32


def at_least_triangles(results):
    for key, r in results.items():
        if key[0] == "simplify":
            assert np.diff(r[0].loop_start.astype(np.int64)).min(initial=3) >= 3, key


@pytest.fixture(scope="module")
def grid():
    """seed -> (the stack, every twin's result on it); nothing is skipped or filtered, and a twin that raises fails every test here."""
    return {seed: (c, LC.run_twins(c)) for seed, c in ((s, LC.grid_loops(s)) for s in LC.SEEDS)}


def test_the_generator_is_the_one_that_was_swept():
    """Seed 0's first loops, drawn by hand from numpy's default_rng in the order n, coordinates, r: pins the order of the draws."""
    rng = np.random.default_rng(0)
    n = int(rng.integers(3, 9))
    first = rng.integers(0, 9, (n, 2)).astype(F)
    r = int(rng.integers(0, 6))
    c = LC.grid_loops(0)
    assert len(c.loop_layer) == 12 and c.n_layers == 3 and c.loop_start[1] == n and (np.diff(c.loop_layer.astype(np.int64)) >= 0).all()
    if r > 2:
        assert c.xy[:n].tobytes() == first.tobytes()
    assert c.keys.tolist() == [7 * v + 1 for v in range(len(c.xy))]
    assert c.xy.min() >= 0 and c.xy.max() <= 8 and (c.xy == np.round(c.xy)).all()


def test_every_twin_runs_on_every_seed(grid):
    assert sorted(grid) == list(range(64))
    for seed, (c, results) in grid.items():
        at_least_triangles(results)
        assert len(results) == 2 + len(LC.SIMPLIFIES) + len(LC.HATCHES) + len(LC.SKINS) + len(LC.OFFSETS), seed


def test_every_twin_runs_on_the_hand_cases_the_tall_stack_and_the_boundary_sizes():
    hand, boundary = LC.hand_cases(), LC.boundary_cases()
    assert len(hand) == 10 and len(boundary) == 10
    for name, c in hand.items():
        at_least_triangles(LC.run_twins(c, hand=True))
    for name, c in boundary.items():
        at_least_triangles(LC.run_twins(c))
    for name in ("tiles 32 x 32", "tiles 33 x 17"):
        o = O.offset(boundary[name], *LC.TILE_INSETS)
        assert (o.stats["nx"], o.stats["ny"]) == ((32, 32) if "32" in name else (33, 17)) and o.stats["n_loops"] >= 4
    tall = LC.run_twins(LC.tall_stack(), tall=True)
    at_least_triangles(tall)
    # the tall stack's layers differ in class: with a window of 1 the layers 64 and 256 carry more than one class, and every occupied
    # layer is filled; the widest window makes every piece both top and bottom skin
    k = tall["skin", 0]
    for l in (64, 256):
        assert len(set(k.cls[k.layer_start[l]:k.layer_start[l + 1]].tolist())) > 1, l
    filled = np.flatnonzero(np.diff(k.layer_start.astype(np.int64)))
    assert filled.tolist() == list(LC.TALL_OCCUPIED)
    assert (tall["skin", len(LC.SKINS)].cls == 3).all()
    assert np.flatnonzero(tall["measures"][1]["n_loops"]).tolist() == list(LC.TALL_OCCUPIED)


def test_a_census_of_what_the_seeds_reach(grid):
    """Lower bounds on what the inputs contain (none is a tolerance): each is a state that no other contour test reaches on the device."""
    zero = {k: 0 for k in range(len(LC.HATCHES))}
    skin_zero, n_class = 0, [0] * 4
    plus_zero = minus_zero = saddles = 0
    area_zero = area_negative = ties = 0
    for seed, (c, results) in grid.items():
        for k in zero:
            zero[k] += results["hatch", k].stats["zero_length"]
            lay, line, uc, tail = results["hatch", k].records
            same_line = (lay[1:] == lay[:-1]) & (line[1:] == line[:-1])
            ties += int((same_line & (uc[1:] == uc[:-1]) & (tail[1:] != tail[:-1])).sum())
        for k in range(len(LC.SKINS)):
            st = results["skin", k].stats
            skin_zero += st["zero_length"]
            n_class = [a + b for a, b in zip(n_class, st["n_class"])]
        for k in range(len(LC.OFFSETS)):
            o = results["offset", k]
            saddles += o.stats["saddle_cells"]
            for D in o.D:
                plus_zero += int(((D == 0) & ~np.signbit(D)).sum())
                minus_zero += int(((D == 0) & np.signbit(D)).sum())
        area = results["measures"][0]["area"]
        area_zero += int((area == 0).sum())
        area_negative += int((area < 0).sum())
    print("zero_length by hatch", zero, "skin", skin_zero, "classes", n_class, "+0.0", plus_zero, "-0.0", minus_zero, "saddles", saddles,
          "areas 0 / < 0", area_zero, area_negative, "ties", ties)
    assert zero[0] > 0 and zero[1] > 0                       # under AXIS and under DIAG
    assert skin_zero > 0 and min(n_class) > 0
    assert plus_zero > 0 and minus_zero > 0
    assert saddles > 0
    assert area_zero > 0 and area_negative > 0
    assert ties > 0


def test_negative_zeros_make_the_order_of_tied_records_visible():
    """Every twin runs on loop_corpus.negative_zeros of the seeds 0 .. 15, and there some records of one line with equal u_c carry
    points of different bytes (+0.0 against -0.0): the only place in this corpus where the order inside a tie group -- (r, j) in the
    skin -- reaches the output. On the plain seeds no such pair exists, which is why they cannot see that order."""
    def pairs(line, uc, bits):
        tied = (line[1:] == line[:-1]) & (uc[1:] == uc[:-1])
        return int((tied & (bits[1:] != bits[:-1]).any(axis=1)).sum())

    def visible(c):
        results = LC.run_twins(c)
        at_least_triangles(results)
        n = 0
        for k in range(len(LC.SKINS)):
            line, uc, r, j, xc, yc = results["skin", k].records
            n += pairs(line, uc, np.stack([xc, yc], axis=1).astype(F).view(np.uint32))
        return n

    plain = sum(visible(LC.grid_loops(seed)) for seed in LC.NEGATIVE_ZERO_SEEDS)
    signed = sum(visible(LC.negative_zeros(LC.grid_loops(seed))) for seed in LC.NEGATIVE_ZERO_SEEDS)
    print("tied records with different points: plain", plain, "with negative zeros", signed)
    assert plain == 0 and signed > 0
    c = LC.negative_zeros(LC.grid_loops(0))
    assert np.signbit(c.xy[c.xy == 0]).all() and (c.xy == 0).any() and c.xy.min() == -4 and c.xy.max() == 4


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_the_doubled_square_cancels():
    """Even-odd: every line crosses the two copies at the same places, so every piece has zero length, and no node is inside."""
    for name in ("doubled", "reversed"):
        c = LC.hand_cases()[name]
        for sp, dirs, off in LC.HATCHES:
            h = H.hatch(c, sp, dirs, off)
            assert h.stats["length"] == 0.0 and h.stats["zero_length"] == h.stats["n_segments"] > 0 and h.layers[0]["length"] == 0.0, (name, sp)
            assert (h.seg[:, :2] == h.seg[:, 2:]).all()
        for res, insets in LC.OFFSETS + (LC.EIGHT_INSETS,):
            o = O.offset(c, res, insets)
            assert o.stats["inside_nodes"] == 0 and not any(np.signbit(D).any() for D in o.D), (name, res)


def test_the_point_loop_s_distance_is_the_distance_to_the_point():
    """Every edge has ee == 0 and takes h = 0: D is the Euclidean distance to the point clamped to the band, +0.0 at the node that is
    the point and positive at every other, never NaN."""
    c = LC.hand_cases()["point"]
    px, py = (float(v) for v in LC.POINT[0])
    for res, insets in LC.OFFSETS + (LC.EIGHT_INSETS,):
        o = O.offset(c, res, insets)
        gx, gy = np.meshgrid(o.xs.astype(np.float64), o.ys.astype(np.float64))
        want = np.minimum(np.sqrt((gx - px) ** 2 + (gy - py) ** 2), float(o.band)).astype(F)
        assert o.D[0].tobytes() == want.tobytes()
        assert not np.signbit(o.D[0]).any() and (o.D[0] > 0).sum() == o.D[0].size - ((gx == px) & (gy == py)).sum()
        assert o.stats["inside_nodes"] == 0
    assert ((gx == px) & (gy == py)).sum() == 1          # (at res 0.5 the point is a node)
    m = S.measures(c)
    assert m[0][0]["area"] == 0 and m[0][0]["length"] == 0 and m[0][0]["bbox"].tolist() == [px, py, px, py]


def test_the_bow_tie_s_hatch_is_inside_by_even_odd():
    """Midpoints of the pieces against an independent even-odd ray cast, wherever they are clear of the edges by a few float32 ulps
    (the form of the check of the traced stacks in tests/test_gpu_offset.py); both lobes are filled."""
    c = LC.hand_cases()["bowtie"]
    loops = c.loops()
    a, b = loops[0], np.roll(loops[0], -1, axis=0)
    ulp = 4 * float(np.abs(c.xy).max()) * 2.0 ** -24
    clear_pieces = 0
    for sp, dirs, off in LC.HATCHES:
        seg = H.hatch(c, sp, dirs, off).seg.astype(np.float64)
        mid = 0.5 * (seg[:, :2] + seg[:, 2:])
        clear = S.seg_dist(mid, a, b) > ulp
        assert H.inside_even_odd(mid[clear], loops).all(), (sp, mid[clear][~H.inside_even_odd(mid[clear], loops)])
        clear_pieces += int(clear.sum())
        if dirs is LC.AXIS:                                   # lines y = 1, 2, 3: one piece in each lobe, x < 2 and x > 2
            assert (mid[clear][:, 0] < 2).any() and (mid[clear][:, 0] > 2).any()
    assert clear_pieces > 10
