"""The numpy twin of the CLEAN contract (tests/cleanref.py; include/gsdf_hip.h, "indexed meshes: clean") held to that contract by
brute force: the derived guarantees (i) .. (iii), the stats' identities and the independence of numbering and face order, on hand
meshes with known answers and on random meshes whose sets collide constantly. No device here."""
from collections import Counter

import numpy as np
import pytest

import cleanref as K
import toporef as T

M, F = K.MERGE_POSITIONS, K.FACES
FLAGS = (M, F, M | F)
NEG0 = np.float32(-0.0)


def soup_of(v, i):
    """An indexed mesh as a soup: three vertices of its own per face, idx = arange."""
    flat = np.asarray(i).astype(np.int64).reshape(-1)
    return np.ascontiguousarray(np.asarray(v, np.float32)[flat]), np.arange(len(flat), dtype=np.uint32).reshape(-1, 3)


def glued_tets():
    """T.TET_V / TET_I and a second tetrahedron (apex (6, 6, 6)) on the other side of its face (1, 2, 3): the inner faces are opposite."""
    v = np.vstack([T.TET_V, [[6, 6, 6]]]).astype(np.float32)
    b = np.array([[1, 3, 2], [3, 1, 4], [2, 3, 4], [1, 2, 4]], np.uint32)     # outward, closed
    return v, np.vstack([T.TET_I, b]).astype(np.uint32), b


def hand_cases():
    """name -> (verts, idx): the cases the issue of the clean pass lists, small enough to check by eye."""
    out = {}
    v, i, _ = glued_tets()
    out["glued-tets"] = (v, i)
    out["rotations"] = (T.TET_V, np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 1, 3]], np.uint32))
    out["two-one"] = (T.TET_V, np.array([[0, 1, 2], [0, 2, 1], [1, 2, 0]], np.uint32))
    out["three-none"] = (T.TET_V, np.array([[1, 2, 3], [1, 2, 3], [2, 3, 1]], np.uint32))
    out["minority-first"] = (T.TET_V, np.array([[0, 2, 1], [0, 1, 2], [1, 2, 0]], np.uint32))
    out["cube-soup"] = soup_of(*T.cube(0, 6))
    v, i = soup_of(T.TET_V, T.TET_I)
    v[0, 0] = NEG0            # slot 0 is vertex 0 = (0, 0, 0): the class's smallest member has a -0 ...
    v[4] = [6, NEG0, NEG0]    # ... and a later copy of vertex 1 = (6, 0, 0) has two, its smallest member (slot 2) none
    out["zero-twins"] = (v, i)
    nan, inf = np.nan, np.inf
    v = np.array([[nan, 0, 0], [nan, 0, 0], [inf, 0, 0], [inf, 0, 0], [0, -inf, 0], [0, -inf, 0], [1, 2, 3], [1, 2, 3], [0, 0, 6]], np.float32)
    out["nonfinite"] = (v, np.array([[0, 2, 4], [1, 3, 5], [6, 0, 8], [7, 1, 8], [6, 8, 2]], np.uint32))
    v = np.array([[0, 0, 0], [0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6]], np.float32)
    out["merge-degenerates"] = (v, np.array([[0, 1, 2], [0, 2, 3], [1, 3, 2], [0, 2, 4], [3, 3, 4]], np.uint32))
    v = np.vstack([[[0, 6, 0]], T.TET_V, [[6, 0, 0], [9, 9, 9], [9, 9, 9]]]).astype(np.float32)      # 0, 5, 6, 7: no face names them
    out["unused-merge"] = (v, (T.TET_I + np.uint32(1)).astype(np.uint32))
    out["all-cancel"] = (T.TET_V, np.array([[0, 1, 2], [0, 2, 1], [1, 3, 2], [2, 3, 1], [3, 3, 0]], np.uint32))
    return out


# ---- brute force, with dictionaries ------------------------------------------------------------------------------------------------
def brute_classes(v, flags):
    cls, seen = [], {}
    for n, p in enumerate(np.ascontiguousarray(v, np.float32).view(np.uint32).tolist()):
        w = tuple(0 if x == 0x80000000 else x for x in p)
        if not flags & M or any((x & 0x7fffffff) >= 0x7f800000 for x in w):
            cls.append(n)
        else:
            cls.append(seen.setdefault(w, n))
    return cls


def is_plus(a, b, c):
    lo, mid, hi = sorted((a, b, c))
    return (a, b, c) in ((lo, mid, hi), (mid, hi, lo), (hi, lo, mid))


def pair_balance(faces):
    """{(p, q), p < q: uses as (p, q) minus uses as (q, p)} over non-degenerate faces, zeros left out."""
    bal = Counter()
    for a, b, c in faces:
        if a == b or b == c or a == c:
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            bal[(min(p, q), max(p, q))] += 1 if p < q else -1
    return {e: n for e, n in bal.items() if n}


def canonical(faces):
    """Faces as a sorted list of triples, each rotated to begin with its smallest entry."""
    rot = []
    for a, b, c in faces:
        k = (a, b, c).index(min(a, b, c))
        rot.append(((a, b, c) * 2)[k:k + 3])
    return sorted(rot)


def brute_stats(v, i, flags):
    cls = brute_classes(v, flags)
    m = [tuple(cls[x] for x in f) for f in np.asarray(i).astype(np.int64).tolist()]
    nd = [f for f in m if len(set(f)) == 3]
    st = {"n_verts_in": len(v), "n_tris_in": len(m), "merged_verts": sum(c != n for n, c in enumerate(cls)), "degenerate": len(m) - len(nd),
          "face_sets": 0, "cancelled_sets": 0, "duplicate_faces": 0, "opposite_faces": 0, "largest_set": 0}
    kept = len(nd)
    if flags & F:
        sets = {}
        for f in nd:
            fr = sets.setdefault(tuple(sorted(f)), [0, 0])
            fr[0 if is_plus(*f) else 1] += 1
        kept = sum(f != r for f, r in sets.values())
        st.update(face_sets=len(sets), cancelled_sets=sum(f == r for f, r in sets.values()), largest_set=max([f + r for f, r in sets.values()], default=0),
                  opposite_faces=sum(2 * min(f, r) for f, r in sets.values()), duplicate_faces=sum(abs(f - r) - 1 for f, r in sets.values() if f != r))
    st["n_tris"] = kept
    return st, cls, m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def check_contract(v, i, flags):
    """Everything the contract promises of clean(v, i, flags), through the twin; returns the twin's result (None: nothing kept)."""
    v = np.ascontiguousarray(v, np.float32)
    i = np.ascontiguousarray(i, np.uint32)
    want, cls, m = brute_stats(v, i, flags)
    ident = np.arange(len(v), dtype=np.uint64)                     # keys = the vertex's own number: a result vertex says where it is from
    nrm = (v[:, ::-1] + np.float32(1)).astype(np.float32)
    dry = K.clean(v, i, ident, nrm, flags, dry=True)
    assert dry[:4] == (None, None, None, None)
    st = dry[4]
    assert {f: st[f] for f in want} == want, (st, want)
    assert st["n_tris"] == st["n_tris_in"] - st["degenerate"] - st["duplicate_faces"] - st["opposite_faces"] and st["opposite_faces"] % 2 == 0
    assert len(K.stats_bytes(st)) == 88 and list(st) == K.STAT_FIELDS
    if st["n_tris"] == 0:
        assert st["n_verts"] == 0
        with pytest.raises(K.CleanError) as e:
            K.clean(v, i, ident, nrm, flags)
        assert e.value.code == K.EMPTY_BUFFERS
        return None
    v2, i2, k2, n2, st2 = K.clean(v, i, ident, nrm, flags)
    assert st2 == st and (len(v2), len(i2)) == (st["n_verts"], st["n_tris"]) and i2.dtype == np.uint32
    # 4: the data of the class's smallest member, bit for bit; numbered by first appearance; kept faces in their order
    src = k2.astype(np.int64)
    assert all(cls[s] == s for s in src) and (bits(v2) == bits(v[src])).all() and (bits(n2) == bits(nrm[src])).all()
    flat = i2.reshape(-1).astype(np.int64)
    firsts = [int(np.flatnonzero(flat == n)[0]) for n in range(len(v2))]
    assert firsts == sorted(firsts) and sorted(set(flat.tolist())) == list(range(len(v2)))
    back = [tuple(int(src[x]) for x in f) for f in i2.tolist()]    # the result's faces over the input's class numbers
    pos, found = 0, 0
    for f in back:                                                  # a subsequence of the merged input faces, not rotated
        pos = m.index(f, pos) + 1
        found += 1
    assert found == len(i2)
    if not flags & F:
        assert back == [f for f in m if len(set(f)) == 3]
    # (i)
    again = K.clean(v2, i2, k2, n2, flags)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:4], (v2, i2, k2, n2)))
    assert [again[4][f] for f in ("merged_verts", "degenerate", "duplicate_faces", "opposite_faces", "cancelled_sets")] == [0] * 5
    # (ii)
    if flags & F:
        assert len({tuple(sorted(f)) for f in back}) == len(back) == st["face_sets"] - st["cancelled_sets"]
    # (iii)
    if st["duplicate_faces"] == 0:
        assert pair_balance(back) == pair_balance(m)
    return v2, i2, k2, n2, st


def check_relabelled(v, i, flags, seed):
    """Permuted faces / renumbered vertices: the same stats, and the same faces over class keys (rotation and order aside)."""
    v = np.ascontiguousarray(v, np.float32)
    i = np.asarray(i).astype(np.int64)
    ckey = np.array(brute_classes(v, flags), np.uint64)             # one key per class, whoever its smallest member is
    base = K.clean(v, i, ckey, None, flags, dry=True)[4]
    rng = np.random.default_rng(seed)
    fp = rng.permutation(len(i))
    vp = rng.permutation(len(v))                                    # new number of old vertex j: vp[j]
    v2, k2 = np.empty_like(v), np.empty_like(ckey)
    v2[vp], k2[vp] = v, ckey
    runs = [(v, i[fp], ckey), (v2, vp[i], k2), (v2, vp[i[fp]], k2)]
    if base["n_tris"] == 0:
        for a, b, c in runs:
            assert K.clean(a, b, c, None, flags, dry=True)[4] == base
        return
    _, i0, k0, _, _ = K.clean(v, i, ckey, None, flags)
    want = canonical(k0[i0.astype(np.int64)].tolist())
    for a, b, c in runs:
        _, i1, k1, _, s1 = K.clean(a, b, c, None, flags)
        assert s1 == base and canonical(k1[i1.astype(np.int64)].tolist()) == want


def all_inputs():
    out = dict(hand_cases())
    out.update({"topo-" + n: m for n, m in T.hand_meshes().items()})
    return out


@pytest.mark.parametrize("name", sorted(all_inputs()))
def test_hand_inputs(name):
    v, i = all_inputs()[name]
    for flags in FLAGS:
        check_contract(v, i, flags)
        check_relabelled(v, i, flags, 5)


def test_glued_tets_cancel_to_one_closed_shell():
    v, i, b = glued_tets()
    v2, i2, _, _, st = check_contract(v, i, F)
    assert (st["cancelled_sets"], st["opposite_faces"], st["duplicate_faces"], st["n_tris"], st["n_verts"]) == (1, 2, 0, 6, 5)
    rep = T.analyse(v2, i2)["report"]
    parts = T.analyse(T.TET_V, T.TET_I)["report"]["volume"] + T.analyse(v, b)["report"]["volume"]
    assert rep["closed_oriented"] == 1 and rep["n_shells"] == 1 and rep["euler"] == 2 and rep["volume"] == parts == 108.0
    before = T.analyse(v, i)["report"]
    assert (before["nonmanifold_edges"], rep["nonmanifold_edges"]) == (3, 0)


def test_which_face_is_kept():
    c = hand_cases()
    _, i2, k2, _, st = check_contract(*c["rotations"], F)
    assert (k2[i2.astype(np.int64)].tolist(), st["duplicate_faces"], st["opposite_faces"], st["largest_set"]) == ([[0, 1, 2], [0, 1, 3]], 2, 0, 3)
    _, i2, k2, _, st = check_contract(*c["two-one"], F)
    assert (k2[i2.astype(np.int64)].tolist(), st["duplicate_faces"], st["opposite_faces"]) == ([[0, 1, 2]], 0, 2)
    _, i2, k2, _, st = check_contract(*c["three-none"], F)
    assert (k2[i2.astype(np.int64)].tolist(), st["duplicate_faces"], st["opposite_faces"], st["face_sets"]) == ([[1, 2, 3]], 2, 0, 1)
    _, i2, k2, _, st = check_contract(*c["minority-first"], F)      # face 0 is the set's smallest, and of the minority
    assert (k2[i2.astype(np.int64)].tolist(), st["duplicate_faces"], st["opposite_faces"]) == ([[0, 1, 2]], 0, 2)


def test_soups_merge():
    c = hand_cases()
    v2, i2, _, _, st = check_contract(*c["cube-soup"], M)
    rep = T.analyse(v2, i2)["report"]
    assert (st["n_verts"], st["merged_verts"], st["n_tris"]) == (8, 28, 12) and rep["closed_oriented"] == 1 and rep["euler"] == 2 and rep["volume"] == 216.0
    v, i = c["zero-twins"]
    v2, i2, k2, _, st = check_contract(v, i, M)
    assert (st["n_verts"], st["merged_verts"]) == (4, 8) and T.analyse(v2, i2)["report"]["closed_oriented"] == 1
    assert k2.tolist() == [0, 1, 2, 5]                              # slots 1, 2 are vertices 2, 1 of the tetrahedron; 5 is its vertex 3
    assert bits(v2).tolist() == bits(v[[0, 1, 2, 5]]).tolist() and bits(v2)[0, 0] == 0x80000000 and (bits(v2)[2] == bits(np.array([6, 0, 0], np.float32))).all()
    v, i = c["nonfinite"]
    _, _, k2, _, st = check_contract(v, i, M)
    assert st["merged_verts"] == 1 and sorted(k2.tolist()) == [0, 1, 2, 3, 4, 5, 6, 8]      # 7 joins 6; no NaN or infinite vertex merges


def test_merge_side_effects():
    c = hand_cases()
    for flags, want in ((F, (1, 0, 4)), (M, (2, 1, 3)), (M | F, (2, 1, 1))):
        st = check_contract(*c["merge-degenerates"], flags)[4]
        assert (st["degenerate"], st["merged_verts"], st["n_tris"]) == want, (flags, st)
    v, i = c["unused-merge"]
    _, _, k2, _, st = check_contract(v, i, M)
    assert st["merged_verts"] == 3 and sorted(k2.tolist()) == [0, 1, 2, 4]       # the used vertex 3 goes by its unused twin 0; 5 joins 2, 7 joins 6
    assert check_contract(v, i, F)[4]["n_verts"] == 4


def test_everything_cancels_and_bad_flags():
    v, i = hand_cases()["all-cancel"]
    assert check_contract(v, i, F) is None and check_contract(v, i, M | F) is None
    st = K.clean(v, i, None, None, F, dry=True)[4]
    assert (st["n_tris"], st["n_verts"], st["cancelled_sets"], st["opposite_faces"], st["degenerate"]) == (0, 0, 2, 4, 1)
    assert check_contract(v, i, M)[4]["n_tris"] == 4
    for flags in (0, 4, 7, 8 | F):
        for dry in (False, True):
            with pytest.raises(K.CleanError) as e:
                K.clean(v, i, None, None, flags, dry=dry)
            assert e.value.code == K.BAD_ARGUMENT


def random_mesh(seed):
    """Indices over a pool of at most 12 vertices whose positions come from a few points (-0 twins and non-finite ones among them)."""
    rng = np.random.default_rng(seed)
    points = np.array([[0, 0, 0], [NEG0, 0, NEG0], [6, 0, 0], [0, 6, 0], [0, 0, 6], [6, 6, 0], [6, NEG0, 0], [np.nan, 0, 0], [0, np.inf, 0], [3, 3, 3]], np.float32)
    n_v = int(rng.integers(3, 13))
    v = points[rng.integers(0, len(points), n_v)]
    i = rng.integers(0, n_v, (int(rng.integers(1, 40)), 3)).astype(np.uint32)
    return v, i


def test_random_meshes():
    seen = Counter()
    for seed in range(200):
        v, i = random_mesh(seed)
        for flags in FLAGS:
            got = check_contract(v, i, flags)
            check_relabelled(v, i, flags, seed)
            st = K.clean(v, i, None, None, flags, dry=True)[4]
            for f in ("merged_verts", "degenerate", "cancelled_sets", "duplicate_faces", "opposite_faces"):
                seen[f] += st[f] > 0
            seen["empty"] += got is None
    assert all(seen[f] >= 20 for f in ("merged_verts", "degenerate", "cancelled_sets", "duplicate_faces", "opposite_faces")), seen
