"""bench.py's plain run and --dump-outputs: the sample it keeps is fixed by the seed and fits the
64 MB budget; on the GPU a plain run prints the headline line without the --full legs, and its dump
is the decode's own output, identical from run to run."""
import json
import os

import numpy as np
import pytest

import bench

DUMP_BUDGET = 64 << 20


def test_sample_index_is_fixed_sorted_and_keeps_both_ends():
    n = 10**9
    a, b = bench.sample_index(n, 7), bench.sample_index(n, 7)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert not np.array_equal(a, bench.sample_index(n, 8))
    assert a[0] == 0 and a[-1] == n - 1 and np.all(np.diff(a) >= 0)
    assert np.array_equal(a[:1 << 16], np.arange(1 << 16))
    assert np.array_equal(a[-(1 << 16):], np.arange(n - (1 << 16), n))
    assert len(a) == (1 << 20) + (2 << 16)
    small = bench.sample_index(1000, 7)
    assert np.array_equal(small, np.arange(1000))  # a small output is kept whole
    assert len(bench.sample_index(0, 7)) == 0


def test_dump_sizes_fit_the_budget():
    """Largest dumps: int64 values as two float64 halves (configs 3, 4), def levels + int32 values
    (config 2), and config 5's two row groups of 11 columns (2 of them with offsets)."""
    per = len(bench.sample_index(10**9, 0))
    assert 2 * 8 * per <= DUMP_BUDGET and (4 + 8) * per <= DUMP_BUDGET
    per5 = len(bench.sample_index(1 << 23, 0, k=1 << 17, edge=1 << 14))
    assert 2 * (11 * (4 + 4) + 2 * 8) * per5 <= DUMP_BUDGET


def test_full_and_dump_options_parse():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "300000", "--page-values", "65536"]


def _plain_run(capsys, extra):
    bench.main(SMALL + extra)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(capsys):
    res = _plain_run(capsys, [])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert res[key] is not None, key
    assert res["unit"] == "levels/s" and res["steps"] == 2 and res["full"] is False
    assert abs(res["value"] - 300000 / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    for key in ("configs", "variants", "cpu_baseline", "pcie_inclusive", "copy_ceiling_gbs", "stages_ms"):
        assert key not in res, key


@pytest.mark.gpu
@pytest.mark.parametrize("config,p_null", [("levels", 0.3), ("dict", 0.0), ("delta", 0.0)])
def test_dump_outputs_is_the_decode_and_repeats(capsys, tmp_path, config, p_null):
    import torch
    import pqgpu
    argv = ["--config", config, "--p-null", str(p_null)]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    _plain_run(capsys, argv + ["--dump-outputs", d1])
    _plain_run(capsys, argv + ["--dump-outputs", d2])
    got, again = _load(d1), _load(d2)
    assert sorted(got) == sorted(again)
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, again[name]), name
    assert sum(a.nbytes for a in got.values()) <= DUMP_BUDGET

    # the same workload decoded here: at this size the sample is every element
    args = bench.parse(SMALL + argv)
    w = bench.Workload(pqgpu, args, 0, config, p_null=p_null if config == "levels" else None)
    ctx = pqgpu.Context(0)
    try:
        bench.decode_once(ctx, w, torch.cuda.current_stream().cuda_stream)
        st, bad = ctx.sync()
        assert st == 0, (st, bad, ctx.error_message())
        nv = int(w.out.num_values)
        raw = w.d_val[:nv * w.es].cpu().numpy()
        if config == "levels":
            assert sorted(got) == ["def_levels", "values"]
            lv = w.d_def[:w.levels].cpu().numpy()
            assert 0 < nv < w.levels  # nulls present: values are the non-null levels only
            assert np.array_equal(got["def_levels"], lv.astype(np.float32))
            assert np.array_equal(got["values"], raw.view(np.int32).astype(np.float64))
        else:
            assert sorted(got) == ["values_hi", "values_lo"]
            back = (got["values_hi"].astype(np.int64) << 32) | got["values_lo"].astype(np.int64)
            assert np.array_equal(back, raw.view(np.int64))
    finally:
        ctx.close()
