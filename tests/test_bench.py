"""bench.py driver contract: ``--gpus N`` runs N ranks (spawned by bench.py
itself when there is no torchrun environment), prints one JSON line from
rank 0, and the strip run reaches the same dt as one rank (gloo, CPU);
``--dump-outputs DIR`` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--backend", "cpu", "--nx", "120", "--ny", "30", "--steps", "6", "--warmup", "2"]


def _run(extra, env_over=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_over or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, env=env,
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r.returncode, lines, r.stderr


def test_bench_gpus_n_launches_n_ranks(hf):
    rc1, l1, err1 = _run([])
    rc4, l4, err4 = _run(["--gpus", "4"])
    assert rc1 == 0 and len(l1) == 1, err1
    assert rc4 == 0 and len(l4) == 1, err4
    one, four = json.loads(l1[0]), json.loads(l4[0])
    assert one["ranks"] == 1 and four["ranks"] == 4
    assert four["config"]["parallelism"] == "strip4"
    assert four["final_dt"] == one["final_dt"] and four["final_time"] == one["final_time"]
    assert four["steps"] == 6 and four["warmup"] == 2


def _load_dump(d):
    import numpy as np

    return {p.stem: np.load(p) for p in sorted(d.iterdir())}


def test_bench_dump_outputs_is_the_state_after_the_last_timed_step(hf, tmp_path):
    """--dump-outputs DIR: one float64 .npy per field, the same bytes from run
    to run, --full or not and with 2 ranks, equal to 2 + 6 steps of the deck."""
    import numpy as np

    import bench
    from openhyperflow2d_amd.models import decks

    rc, l1, err = _run(["--dump-outputs", str(tmp_path / "a")])
    assert rc == 0 and len(l1) == 1, err
    rc, l2, err = _run(["--full", "--gpus", "2", "--dump-outputs", str(tmp_path / "b")])
    assert rc == 0 and len(l2) == 1, err
    one, two = json.loads(l1[0]), json.loads(l2[0])
    assert one["steps"] == 6 and one["ms_per_step"] > 0 and one["dtype"] == "fp64"
    assert two["final_dt"] == one["final_dt"] and two["final_time"] == one["final_time"]
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    assert sorted(a) == sorted(bench.DUMP_FIELDS + ["dt_time"]) == sorted(b)
    sim = hf.Simulation(decks.wedge15(120, 30, nmax=10 ** 9, nout=10 ** 8), "cpu", lean=True)
    sim.step(2)
    sim.step(6)
    for name in bench.DUMP_FIELDS:
        assert a[name].dtype == np.float64 and a[name].shape == (120, 30)
        assert a[name].tobytes() == b[name].tobytes(), name
        assert a[name].tobytes() == sim.field(name).tobytes(), name
    assert a["dt_time"].tolist() == [one["final_dt"], one["final_time"]] == b["dt_time"].tolist()
    assert np.isfinite(a["S0"]).all() and a["S0"].max() > 1.0 and np.ptp(a["S0"][a["S0"] > 0]) > 0   # 0: the wedge


def test_bench_dump_outputs_samples_a_grid_past_the_budget(tmp_path, monkeypatch):
    """Fields past DUMP_BYTES are written as one fixed seeded sample of cells."""
    import numpy as np

    import bench

    class Sim:
        world = 1

        class solver:
            download = staticmethod(lambda: None)

        class case:
            @staticmethod
            def field(name):
                return np.arange(7 * 11, dtype=np.float64).reshape(7, 11) + bench.DUMP_FIELDS.index(name) * 100.0

    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 8 * (len(bench.DUMP_FIELDS) + 1) * (64 + 20))
    for d in ("a", "b"):
        bench.dump_outputs(Sim, 0, str(tmp_path / d), {"dt": 0.5, "time": 2.0})
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    cells = a["sample_cells"]
    assert cells.dtype == np.float64 and cells.shape == (20,) and len(set(cells.tolist())) == 20
    assert (np.diff(cells) > 0).all() and cells.min() >= 0 and cells.max() < 77
    for k, name in enumerate(bench.DUMP_FIELDS):
        assert a[name].tolist() == (cells + 100.0 * k).tolist() == b[name].tolist()
    assert a["dt_time"].tolist() == [0.5, 2.0]


@pytest.mark.gpu
def test_bench_gpu_dump_matches_the_cpu_stepper(gpu, tmp_path):
    """A plain GPU run (autotune, priming and all) dumps the state its last
    timed step left: the CPU stepper reaches the same one after as many steps
    (bound: smoke()'s 1e-10 of the field's maximum)."""
    import numpy as np

    import bench
    from openhyperflow2d_amd.models import decks

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nx", "200", "--ny", "40",
                        "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "g")],
                       capture_output=True, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr
    rec = json.loads(lines[0])
    assert rec["config"]["backend"] == "gpu" and rec["config"]["kernel"] == "lean" and rec["steps"] == 4
    g = _load_dump(tmp_path / "g")
    cpu = gpu.Simulation(decks.wedge15(200, 40, nmax=10 ** 9, nout=10 ** 8), "cpu")
    cpu.step(rec["warmup"] + rec["prime_steps"] + rec["steps"])
    assert g["dt_time"][1] == pytest.approx(cpu.summary()["time"], rel=1e-12)
    for name in bench.DUMP_FIELDS:
        want = cpu.field(name)
        err = float(np.abs(g[name] - want).max())
        print("%s: max abs diff %.3e, field max %.3e" % (name, err, float(np.abs(want).max())))
        assert g[name].shape == (200, 40) and np.isfinite(g[name]).all()
        assert err <= 1e-10 * max(float(np.abs(want).max()), 1e-300), name


def test_bench_world_size_mismatch_fails_loudly(hf):
    rc, lines, err = _run(["--gpus", "2"], {"WORLD_SIZE": "1"})
    assert rc != 0 and not lines
    assert "WORLD_SIZE=1" in err
