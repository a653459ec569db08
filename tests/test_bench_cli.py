"""bench.py's command line: the plain run's result line, --dump-outputs and
--full.  The runs are in-process (bench.main() on a 24^3 lattice)."""
import json
import os
import sys

import numpy as np
import pytest

PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "kernel_ms_per_pass", "unit_rates", "final_complex", "cpu_baseline", "small_net",
             "small_net_curve", "large_net", "finish_synth64h"}


def _bench(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, lines  # the result line alone on stdout
    return json.loads(lines[0])


def test_dump_sample_rows_are_fixed():
    import bench
    assert bench.sample_rows(bench.DUMP_ROWS, 0) is None  # kept whole
    n = 3 * bench.DUMP_ROWS + 17
    a, b = bench.sample_rows(n, 0), bench.sample_rows(n, 0)
    assert np.array_equal(a, b) and a.shape == (bench.DUMP_ROWS,)
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) > 0)  # sorted, distinct, in range
    assert not np.array_equal(a, bench.sample_rows(n, 1))  # vertices and edges: separate streams


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(cuda, monkeypatch, capsys, tmp_path):
    """A plain run prints the headline keys and none of --full's; its dump is
    the last timed pass's complex, identical from run to run and equal to
    what the engine exports after a pass over the same net."""
    import bench
    import torch
    from tropical._engine import engine_for
    from tropical.distributed import complex_hash
    args = ("--gpus", "1", "--steps", "3", "--warmup", "1", "--marks", "24")
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    out = _bench(monkeypatch, capsys, *args, "--dump-outputs", d1)
    assert PLAIN_KEYS <= set(out) and not FULL_ONLY & set(out), sorted(out)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["edges_subdivided_per_pass"] / (out["ms_per_step"] * 1e-3),
                                         rel=1e-2)
    _bench(monkeypatch, capsys, *args, "--dump-outputs", d2)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) == ["complex.npy", "edges.npy", "step_stats.npy", "vertices.npy"]
    got = {n[:-4]: np.load(os.path.join(d1, n)) for n in names}
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(d2, n))), n
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    eng = engine_for(bench.make_net(24, cuda, 6))
    stats = []
    eng.lattice_box([0, 0, 0], [23, 23, 23])
    eng.run_steps(stats)
    V, E, _ = eng.export()
    torch.cuda.synchronize(cuda)
    assert np.array_equal(got["vertices"], V.cpu().numpy())
    assert np.array_equal(got["edges"], E.cpu().numpy().astype(np.float64))
    hv, he = complex_hash(V, E)
    c = [int(x) for x in got["complex"]]
    assert (c[0], c[1]) == (V.shape[0], E.shape[0])
    assert ((c[2] << 32) | c[3], (c[4] << 32) | c[5]) == (hv & (2 ** 64 - 1), he & (2 ** 64 - 1))
    assert got["step_stats"].shape[0] == len(stats) == out["active_steps"]
    assert got["step_stats"][:, 3].sum() == sum(s["S"] for s in stats)  # column 3: S (TnpStepStats)


@pytest.mark.gpu
def test_full_run_adds_the_kernel_pass_and_the_final_complex(cuda, monkeypatch, capsys):
    """--full (here without the CPU baseline and the legs) reports what a
    plain run leaves out, with the headline keys unchanged."""
    out = _bench(monkeypatch, capsys, "--gpus", "1", "--steps", "2", "--warmup", "1", "--marks", "24",
                 "--full", "--no-cpu")
    assert PLAIN_KEYS <= set(out)
    assert {"roofline", "kernel_ms_per_pass", "unit_rates", "final_complex"} <= set(out)
    assert out["kernel_ms_per_pass"] and out["final_complex"]["vertices"] > 0
