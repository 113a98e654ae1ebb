"""bench.py's command line and its --dump-outputs writer, without a GPU: what a plain run leaves out, what --full keeps, how many
timed regions each one has, and what the dump holds (name, float32, the size cap and its seeded row sample)."""
import os

import numpy as np
import pytest

import bench


def test_a_plain_run_is_the_headline_alone():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2
    assert a.single_mode and a.no_cpu_baseline and a.no_configs and a.no_entry_points and a.no_kernel_events
    assert not a.spans and not a.h2d
    assert bench.timed_regions(a) == 1                      # exactly K timed steps
    assert bench._live_pmc_passes(["--steps", "7"]) is None  # no profiler passes either


def test_full_keeps_every_leg_and_the_no_options_still_apply():
    a = bench.parse_args(["--full"])
    assert not (a.single_mode or a.no_cpu_baseline or a.no_configs or a.no_entry_points or a.no_kernel_events)
    assert a.spans and a.h2d
    assert bench.timed_regions(a) == bench.REGIONS
    assert bench.timed_regions(bench.parse_args(["--full", "--eager"])) == 1
    b = bench.parse_args(["--full", "--no-configs", "--no-h2d"])
    assert b.no_configs and not b.h2d and not b.no_cpu_baseline


def test_options_are_not_abbreviated():
    """The PMC passes are decided from the literal spellings in argv before argparse runs: a prefix must not mean --full."""
    with pytest.raises(SystemExit):
        bench.parse_args(["--ful"])


def test_dump_outputs_is_refused_with_a_dry_launch():
    with pytest.raises(SystemExit):
        bench.parse_args(["--dry-launch", "--dump-outputs", "out"])


def test_dump_outputs_writes_float32(tmp_path):
    a = np.random.default_rng(3).standard_normal((64, 1024))
    bench.dump_outputs(str(tmp_path / "d"), {"fused_av_embedding": a})
    got = np.load(tmp_path / "d" / "fused_av_embedding.npy")
    assert got.dtype == np.float32 and got.shape == a.shape
    assert np.array_equal(got, a.astype(np.float32))


def test_dump_outputs_caps_the_size_with_a_fixed_seeded_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 1024 * 4)       # 16 of the 64 rows fit
    a = np.arange(64 * 1024, dtype=np.float32).reshape(64, 1024)
    b = -a
    for d, x in (("a", a), ("a2", a), ("b", b)):
        bench.dump_outputs(str(tmp_path / d), {"fused_av_embedding": x})
    ga, ga2, gb = (np.load(tmp_path / d / "fused_av_embedding.npy") for d in ("a", "a2", "b"))
    assert ga.nbytes <= bench.DUMP_LIMIT_BYTES and ga.shape == (16, 1024)
    rows = ga[:, 0].astype(np.int64) // 1024
    assert np.all(np.diff(rows) > 0) and np.array_equal(ga, a[rows])   # whole rows, in order, no duplicates
    assert np.array_equal(ga, ga2)                                     # the same sample on every run ...
    assert np.array_equal(gb, b[rows])                                 # ... and for every array of that shape
