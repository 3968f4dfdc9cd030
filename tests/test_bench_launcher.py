"""bench.py's own launcher (no GPU needed): `python bench.py --gpus N` without WORLD_SIZE must re-execute itself under
torch.distributed.run with the same arguments; with WORLD_SIZE set it must not. Also the sample --dump-outputs writes, and (GPU)
a plain run with --dump-outputs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_self_launch_builds_the_drivers_command(monkeypatch):
    import subprocess
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "5", "--warmup", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.self_launch(8) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 1024
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "5", "--warmup", "2"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_pmc_summary_prefers_the_running_code_and_says_so():
    import bench
    w = "examples/npt-flange resdiv 1600: octree prune + marching cubes on device (res 0.0541987, 12 levels)"
    any_ = bench.pmc_summary(w, None)
    assert any_ and any_["code_match"] is True and any_["valu_lane_instr_per_eval"] > 0
    other = bench.pmc_summary(w, "not-a-code-key")
    assert other and other["code_match"] is False and other["source"] == any_["source"]
    assert "DIFFERS" in bench.counters_note(other["source"], other["code_match"])
    assert bench.pmc_summary("examples/no-such-scene resdiv 7", None) == {}
    va = bench.valu_roofline(5e11, w, "not-a-code-key")
    assert va["code_match"] is False and 0 < va["frac"] < 1


def test_triangle_sample_is_fixed_and_independent_of_emission_order():
    """--dump-outputs compares two builds output for output: the sample of a triangle set must not depend on the order the device
    emitted it in, must keep to its byte budget, and a triangle more or less must change at most one row."""
    import numpy as np
    import bench
    rng = np.random.default_rng(3)
    tris = rng.random((50000, 3, 3), dtype=np.float32)
    budget = 1 << 18  # ~7300 of the 50000 triangles' 36 B
    a = bench.triangle_sample(tris, budget)
    b = bench.triangle_sample(tris[rng.permutation(len(tris))], budget)
    assert a.dtype == np.float32 and a.shape[1] == 9 and 0 < a.nbytes <= budget
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    u = a.view(np.uint32)
    assert all(tuple(u[i]) < tuple(u[i + 1]) for i in range(len(u) - 1))   # sorted bitwise, no duplicates
    c = bench.triangle_sample(tris[1:], budget)
    assert abs(len(c) - len(a)) <= 1 and len({r.tobytes() for r in a} ^ {r.tobytes() for r in c}) <= 1
    small = tris[:100]                                                        # under the budget: every triangle, sorted
    assert len(bench.triangle_sample(small, budget)) == 100


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps K --dump-outputs DIR`: one JSON line with the headline keys and K timed steps, only the headline's
    measurements (no --full), and the last mesh's triangles and counts under DIR."""
    import json
    import subprocess
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--preheat", "2", "--resdiv", "400",
           "--dump-outputs", str(tmp_path)]
    pr = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in pr.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "sdf_evals_per_s" and d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
    assert abs(d["value"] - d["evals_per_step"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"roofline", "cpu_baseline", "one_shot", "distinct_rows", "host_inclusive"} & set(d)
    counts = np.load(tmp_path / "counts.npy")
    tris = np.load(tmp_path / "triangles.npy")
    assert counts.dtype == np.float64 and counts[0] == 423852 == d["triangles_per_step"]   # README.md:116,130
    assert counts[1] == d["evals_per_step"]
    assert tris.dtype == np.float32 and tris.shape == (423852, 9)                        # 15 MB: every triangle, sorted
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
