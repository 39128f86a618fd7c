"""bench.py's secondary workload lines run end to end on the GPU and print a well-formed line
(one short run each, in-process): one rank of the c4 agent partition (8- and 2-way, every halo
scheme) and the irregular c4-ba graph.  The default c2 line is the driver's own bench run."""
import importlib.util
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod_gpu", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_line(bench, monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert lines, "no JSON line"
    return json.loads(lines[-1])


@pytest.mark.parametrize("rank_of", [8, 2])
def test_c4_rank_line(cuda, bench, monkeypatch, capsys, rank_of):
    d = run_line(bench, monkeypatch, capsys, ["--workload", "c4-rank", "--rank-of", str(rank_of),
                                              "--steps", "3", "--warmup", "1", "--full"])
    assert d["unit"] == "rounds/s" and d["value"] > 0
    assert set(d["schemes"]) == {"whole", "chunks", "split"}
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0.2 < r["frac"] < 1.0, r
    assert 0.2 < d["pack"]["frac"] < 1.0, d["pack"]
    cpu = d["cpu_baseline"]        # this rank's round on one host core, the CPU named
    assert cpu["value"] > 0 and cpu["cores"] == 1 and cpu["host_cpu"], cpu


def test_c4_ba_line(cuda, bench, monkeypatch, capsys):
    d = run_line(bench, monkeypatch, capsys, ["--workload", "c4-ba", "--steps", "2", "--warmup",
                                              "1", "--no-cpu"])
    assert d["unit"] == "rounds/s" and d["value"] > 0
    assert d["config"]["plan"]["path"] == 5 and d["config"]["plan"]["hub_rows"] == 256
    assert 0.2 < d["roofline"]["frac"] < 1.0


def test_plain_c2_line_dumps_its_outputs(cuda, bench, monkeypatch, capsys, tmp_path):
    """A plain run of the headline path at a small shape (64 agents x 4100 columns: more than one
    tile, a ragged last one): the line carries ms_per_step for exactly --steps timed rounds and
    none of --full's extras, and --dump-outputs writes the last timed round's X, dev_sq and
    dev_max as float32 .npy -- the same bits from run to run (seeded inputs), dev_sq the rows'
    own ||x_a - mean||^2 (fp32 fused reduction against numpy in fp64: 1e-5 relative, the bar of
    the mix tests) and dev_max the root of its maximum."""
    import numpy as np
    outs = []
    for k in (0, 1):
        out = tmp_path / f"run{k}"
        d = run_line(bench, monkeypatch, capsys, ["--agents", "64", "--params", "4100", "--steps",
                                                  "3", "--warmup", "1", "--dump-outputs", str(out)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1) < 1e-9    # rounds/s = 1 / step time
        assert d["cpu_baseline"] is None and d["fdla_weights"] is None
        assert d["roofline"]["measured_triad_ceiling_GBs"] is None
        assert sorted(p.name for p in out.iterdir()) == ["X.npy", "dev_max.npy", "dev_sq.npy"]
        outs.append({p.stem: np.load(p) for p in out.iterdir()})
    a, b = outs
    assert a["X"].shape == (64, 4100) and a["dev_sq"].shape == (64,) and a["dev_max"].shape == (1,)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    X = a["X"].astype(np.float64)
    want = ((X - X.mean(axis=0)) ** 2).sum(axis=1)
    assert np.max(np.abs(a["dev_sq"] - want) / want) < 1e-5
    # (one fp32 rounding of the root apart at the most)
    assert abs(a["dev_max"][0] - np.sqrt(a["dev_sq"].max())) <= 2e-7 * a["dev_max"][0]
    assert abs(d["final_max_deviation"] - a["dev_max"][0]) <= 2e-7 * a["dev_max"][0]
    # an output over the size budget is written as the seeded column sample of the same run
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 4 * 1000)
    cols = bench.dump_columns(64, 4100)
    assert cols.shape == (1000,) and np.all(np.diff(cols) > 0) and cols[-1] < 4100
    assert np.array_equal(cols, bench.dump_columns(64, 4100))
    out = tmp_path / "sampled"
    run_line(bench, monkeypatch, capsys, ["--agents", "64", "--params", "4100", "--steps", "3",
                                          "--warmup", "1", "--dump-outputs", str(out)])
    Xs = np.load(out / "X.npy")
    assert Xs.dtype == np.float32
    assert np.array_equal(Xs.view(np.uint32), a["X"][:, cols].view(np.uint32))
    assert np.array_equal(np.load(out / "dev_sq.npy"), a["dev_sq"])
