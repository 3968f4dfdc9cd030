"""Every entry point gives its answer whatever the handle ran before.

The suite holds almost every entry point to the oracle bit for bit, but nearly always on a handle created for that one check. A
program handle carries state from call to call (tests/handle_acts.py lists it), and finished meshes hand their buffers to a pool that
the next mesh of ANY handle takes from. Here the acts of tests/handle_acts.py run after one another on one handle:

  1. every ordered pair (A, B) of acts, error acts included, on a fresh handle of each 3-D tree (and of the 2-D tree): A at a small
     rung and B at a large one and the other way round; A's result object kept alive across B and read again afterwards (its bytes
     must be those of its first read), or closed before B (its buffer comes back through the pool);
  2. long walks: one handle, 150 acts drawn at random, octree meshes as blocking calls or start / wait with up to three in flight
     and Evaluate issued meanwhile, result objects kept in a ring of eight and read again when they leave it;
  3. the same walk on a handle with per-tree kernels, built before the walk or in the background and adopted on the way;
  4. two handles of different trees taking turns, every mesh closed at once: each mesh gets the buffer the other tree's gave back.

Every result is checked twice: against the oracle where the oracle has the answer (canon), and label by label against the same act
on a fresh handle (canon and more). Where the existing tests state what Evaluations() does, it must grow by the act's own count.

An upward step of the ladder asks for a buffer sized by the smaller mesh's hint (handle_acts.takes_rerun): unless the pool hands out
a larger one, the mesh overflows it and is repeated once at the exact size. n_tris, evals and pruned_leaves of such a mesh are in
its canon like any other's: a rerun that counted twice fails there. In a long-lived process the pool keeps its sixteen largest
buffers, so whether a given pair takes the rerun depends on what ran before it; hence

  5. climbs: acts up the ladder on one handle in a fresh process, every result kept alive, where each upward step is certain to
     overflow its first buffer (handle_acts.CLIMBS): octree -> octree, octree -> flat, flat -> octree, flat -> flat, records -> records.
     Dual contouring after dual contouring has no such step at these sizes: its lists start at 2^20 cubes or the whole lattice.

The module has no `pytestmark`: the CPU tests of the table (handle_acts.py, whose name pytest does not collect) are imported below and
must run without a GPU; every other test carries the mark itself.

Size: 30 acts on a 3-D handle (22 uses, 8 error acts) and 6 on the 2-D handle (4 and 2); 900 ordered pairs per 3-D tree and 36 on the 2-D
tree, each at two rung orders with A kept alive and closed (3 600 pair runs per 3-D tree); 6 long walks, 4 walks through per-tree
kernels, 1 walk of two handles, 8 climbs.

Time, one run on one MI355X machine: this file 61 s (75 GPU cases: a pair case of 120 pair runs 0.2-1.1 s, 2-3 s for the ones that first
ask the oracle for 87 383 points or start three meshes at every rung; a long walk 0.3 s; the four per-tree builds side by side 6-11 s;
the eight climbs, a process each, side by side 1.7 s), beside it the rest of the GPU suite 814 s (618 cases).
"""
import collections
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import handle_acts as H
from handle_acts import (test_comparators_are_sensitive, test_every_oracle_backed_expectation_exists,  # noqa: F401 -- collected here
                         test_ladder_counts_are_the_stated_ones, test_no_mesh_exceeds_the_size_bound, test_upward_steps_take_the_rerun_path)
from par import pmap

gpu_test = pytest.mark.gpu
STEPS = 150
# (variant of pair_rungs: 0 small -> large, 1 large -> small; A's result kept alive across B, or closed before it)
COMBOS = ((0, True), (1, False), (0, False), (1, True))

_LOCK = threading.RLock()
_FIXED, _BASE = {}, {}


def fixed_mesh(gpu, t):
    with _LOCK:
        if t.name not in _FIXED:
            _FIXED[t.name] = H.make_fixed(gpu, t)
        return _FIXED[t.name]


def kernel_free(act, d):
    """`d` without the labels that depend on which kernels the handle runs: the evaluations of the share_corners forms."""
    drop = {"+evals", "+evals_leaf"} if getattr(act, "share", 0) else set()
    return {k: v for k, v in d.items() if k not in drop}


def baseline(gpu, t, act, rung):
    """The act's canon and more on a fresh interpreter handle: made once, shared, never written to."""
    key = (t.name, act.name, rung)
    with _LOCK:
        if key not in _BASE:
            cx = H.fresh_ctx(gpu, t, fixed_mesh(gpu, t) if t.dim == 3 else None)
            try:
                r = act.run(cx, rung)
                if act.oracle_backed:
                    H.check(r.canon, act.want(t, rung), (key, "fresh handle against the oracle"))
                _BASE[key] = r.both()
                r.close()
            finally:
                cx.sdf.close()
        return _BASE[key]


def verify(gpu, cx, act, rung, r, what, interp=True):
    if act.oracle_backed:
        H.check(r.canon, act.want(cx.t, rung), (what, "against the oracle"))
    got, base = r.both(), baseline(gpu, cx.t, act, rung)
    if not interp:
        got, base = kernel_free(act, got), kernel_free(act, base)
    H.check(got, base, (what, "against the same act on a fresh handle"))


def run_checked(gpu, cx, act, rung, what, interp=True):
    e0 = cx.sdf.Evaluations()
    r = act.run(cx, rung)
    if r.evals is not None:
        assert cx.sdf.Evaluations() - e0 == r.evals, (what, "Evaluations() grew by", cx.sdf.Evaluations() - e0, "the act evaluated", r.evals)
    verify(gpu, cx, act, rung, r, what, interp)
    return r


def run_pair(gpu, t, a, ra, b, rb, keep):
    what = (t.name, a.name, ra, "then", b.name, rb, "A kept alive" if keep else "A closed first")
    cx = H.fresh_ctx(gpu, t, fixed_mesh(gpu, t) if t.dim == 3 else None)
    try:
        r1 = run_checked(gpu, cx, a, ra, what + ("A",))
        if not keep:
            r1.close()
        r2 = run_checked(gpu, cx, b, rb, what + ("B",))
        for l in (r1.live if keep else []) + r2.live:
            l.reread(what)
        r1.close()
        r2.close()
    finally:
        cx.sdf.close()


def pair_matrix(gpu, tname, acts, first):
    t = H.tree(tname)
    ia = [a.name for a in acts].index(first)
    for ib, b in enumerate(acts):
        for variant, keep in COMBOS:
            ra, rb = H.pair_rungs(ia, ib, variant)
            run_pair(gpu, t, acts[ia], ra, b, rb, keep)


@gpu_test
@pytest.mark.parametrize("first", [a.name for a in H.ACTS3])
@pytest.mark.parametrize("tname", H.TREES3)
def test_every_ordered_pair(gpu, tname, first):
    pair_matrix(gpu, tname, H.ACTS3, first)


@gpu_test
@pytest.mark.parametrize("first", [a.name for a in H.ACTS2])
def test_every_ordered_pair_2d(gpu, first):
    pair_matrix(gpu, H.TREE2, H.ACTS2, first)


# ---------------- climbs: the rerun, for certain ----------------
def climb_main(tname, kind):
    """In a process of its own (handle_acts.CLIMBS says why that makes the overflow certain): the acts of the climb on one handle, each
    held to the oracle -- triangles, n_tris, evals, pruned_leaves: a rerun must not count twice or leave a stale tail -- and every
    result read again at the end. Only this handle exists: a fresh handle to compare with would feed the pool."""
    from gsdf_amd import hip as gpu
    gpu.init(0)
    t = H.tree(tname)
    cx = H.fresh_ctx(gpu, t)
    alive, prev = [], 0
    for name, rung in H.CLIMBS[kind]:
        act = H.BY_NAME[name]
        r = act.run(cx, rung)
        H.check(r.canon, act.want(t, rung), (tname, kind, name, rung, "against the oracle"))
        n = int(np.frombuffer(r.more["records"], np.int64)[0]) if kind.startswith("records") else int(np.frombuffer(r.canon["n_tris"], np.int64)[0])
        assert not prev or H.takes_rerun(prev, n), (tname, kind, name, rung, prev, n)
        print(tname, kind, name, rung, "count", n, "first buffer", H.first_guess(prev))
        alive += [(name, rung, l) for l in r.live]
        prev = n
    for name, rung, l in alive:
        l.reread((tname, kind, name, rung, "at the end of the climb"))
    print("climbed")


@gpu_test
def test_climbs_take_the_rerun_path(gpu):
    """Every climb of handle_acts.CLIMBS on both 3-D trees, each in a fresh process (what the test is about: an empty pool), side by
    side."""
    tests = os.path.dirname(os.path.abspath(__file__))
    cases = [(tname, kind) for tname in H.TREES3 for kind in H.CLIMBS]

    def run(case):
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_handle_history as T; T.climb_main(%r, %r)" % ((os.path.dirname(tests), tests) + case)
        return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    for case, r in zip(cases, pmap(run, cases, workers=len(cases))):
        assert r.returncode == 0 and r.stdout.strip().endswith("climbed"), (case, r.stdout[-2000:], r.stderr[-4000:])
        print(r.stdout)


# ---------------- walks ----------------
REFUSED_IN_FLIGHT = ("flat", "dc", "dcix", "mc")     # the meshers that borrow the octree's first workspace
BESIDE_JOBS = (H.Evaluate, H.Pipelined, H.StaleTicket)  # host-buffer evaluation: issued while octree jobs are in flight


class Walker:
    """One handle in a walk: its jobs in flight and the ring of result objects still alive."""

    def __init__(self, gpu, cx, interp=True, ring=8):
        self.gpu, self.cx, self.interp, self.ring_len = gpu, cx, interp, ring
        self.pending, self.ring = [], collections.deque()
        self.log = []

    def keep(self, r, what):
        for l in r.live:
            self.ring.append((what, l))
        while len(self.ring) > self.ring_len:
            w, l = self.ring.popleft()
            l.reread((w, "leaving the ring at", what))
            l.close()

    def wait_one(self, k, what):
        act, rung, pend, started = self.pending.pop(k)
        r = act.finish(self.cx, pend.wait())
        verify(self.gpu, self.cx, act, rung, r, (what, "job started at", started), self.interp)
        self.keep(r, started)

    def drain(self, rng, what):
        while self.pending:
            self.wait_one(int(rng.integers(len(self.pending))), what)

    def step(self, rng, acts, what):
        act, rung = acts[int(rng.integers(len(acts)))], int(rng.integers(4))
        what = what + (act.name, rung)
        self.log.append(what)
        if type(act) is H.Octree:
            if len(self.pending) == 3:
                self.wait_one(int(rng.integers(3)), what)
            if rng.random() < 0.5:
                self.pending.append((act, rung, act.start(self.cx, rung), what))
                return
        elif not isinstance(act, BESIDE_JOBS):
            if self.pending and act.family in REFUSED_IN_FLIGHT:     # the documented refusal, which changes nothing
                with pytest.raises(self.gpu.HipError) as e:
                    act.run(self.cx, rung)
                assert e.value.code == H.BAD_ARGUMENT and H.IN_FLIGHT in e.value.msg, (what, e.value.code, e.value.msg)
            self.drain(rng, what)
        self.keep(run_checked(self.gpu, self.cx, act, rung, what, self.interp), what)

    def finish(self, rng, what):
        self.drain(rng, what)
        while self.ring:
            w, l = self.ring.popleft()
            l.reread((w, "at the end of", what))
            l.close()


def walk(gpu, walkers, seed, at_step=None, acts=None):
    """STEPS acts, the walkers taking turns; at_step: {step: what to do to the walker before it}."""
    rng = np.random.default_rng(seed)
    acts = acts or H.ACTS3
    for k in range(STEPS):
        w = walkers[k % len(walkers)]
        if at_step and k in at_step:
            at_step[k](w)
        try:
            w.step(rng, acts, (w.cx.t.name, "seed", seed, "step", k))
        except BaseException:
            print("the walk so far:", *w.log[-12:], sep="\n  ")
            raise
    for w in walkers:
        w.finish(rng, (w.cx.t.name, "seed", seed, "end"))


def walker(gpu, tname, fixed=None, interp=True, ring=8):
    t = H.tree(tname)
    return Walker(gpu, H.fresh_ctx(gpu, t, fixed if fixed is not None else fixed_mesh(gpu, t)), interp, ring)


@gpu_test
@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("tname", H.TREES3)
def test_long_walk(gpu, tname, seed):
    w = walker(gpu, tname)
    walk(gpu, [w], seed)
    w.cx.sdf.close()


def _specialised(info):
    return info["specialized"] and any(v.endswith(":specialised") for v in info["kernels"].values())


@gpu_test
def test_walks_through_per_tree_kernels(gpu):
    """The walk on a handle after specialize(), and on one whose build runs in the background from before the first act and is
    waited for at step 75: the same bytes before and after adoption. A build that is refused fails the test. Four compiler runs,
    side by side (tests/par.py); each walk has a fixed mesh of its own."""
    for tname in H.TREES3:                      # the shared expectations first, on this thread
        fixed_mesh(gpu, H.tree(tname))

    def job(case):
        tname, how = case
        t = H.tree(tname)
        with _LOCK:                             # the shared mesh's bytes (a second weld numbers its vertices in its own order)
            fx = gpu.IndexedHIP.from_arrays(*fixed_mesh(gpu, t).read())
        w = walker(gpu, tname, fixed=fx, interp=False)
        sdf = w.cx.sdf
        if how == "before":
            sdf.specialize()
            assert _specialised(sdf.info()), sdf.info()
            walk(gpu, [w], 21)
        else:
            sdf.specialize_async()

            def adopt(wk):
                assert wk.cx.sdf.specialize_poll(wait=True), "the background build did not give per-tree kernels"
            walk(gpu, [w], 22, at_step={75: adopt})
        assert _specialised(sdf.info()), sdf.info()
        sdf.close()
        fx.close()
    pmap(job, [(tname, how) for tname in H.TREES3 for how in ("before", "background")], workers=4)


@gpu_test
def test_two_handles_through_one_pool(gpu):
    """A handle per 3-D tree, taking turns, every result object closed at once (a ring of none): each mesh takes the buffer that
    the other tree's mesh just gave back, with its old contents."""
    ws = [walker(gpu, tname, ring=0) for tname in H.TREES3]
    meshers = [a for a in H.ACTS3 if a.family in H.MESHERS] + [H.BY_NAME["evaluate"], H.BY_NAME["raycast"], H.BY_NAME["project"]]
    walk(gpu, ws, 31, acts=meshers)
    for w in ws:
        w.cx.sdf.close()
