"""bench.py's plain run and --dump-outputs: what a plain run prints, what it writes, and that --full times the same path.
CPU: the dump format on records made up here (sampling, global contig ids, the packed selection unpacked, the size bound).
GPU: a plain run and a --full run of the same small workload write the same records, and the plain line holds no --full field."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench
import cornetto_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("telomere_runs", "telomere_windows", "sdust_intervals", "selected_cov_windows")
FULL_ONLY = ("roofline", "determinism", "cpu_baseline", "parity", "scaling_model", "cold_step_ms_next_assembly", "e2e", "profiles", "reads")


def _records(dt, n, nctg, rng):
    a = np.zeros(n, dtype=dt)
    for c in dt.names:
        a[c] = rng.integers(0, 1 << 30, n)
    a["ctg"] = np.sort(rng.integers(0, nctg, n))
    return a


def _fake_rank(n_hits, n_pk, world=1, rank=0):
    rng = np.random.default_rng(7)
    lens = [250_000_000, 120_000_000, 3_000]
    pk = np.zeros(n_pk, dtype=cornetto_amd.REGPK_DT)
    pk["st"] = np.sort(rng.integers(0, 100_000_000, n_pk))
    pk["depth"], pk["mq_depth"] = rng.integers(0, 65535, n_pk), rng.integers(0, 65535, n_pk)
    ctg_first = np.array([0, n_pk // 2, n_pk, n_pk], dtype=np.int64)
    held = (_records(cornetto_amd.HIT_DT, n_hits, 3, rng), _records(cornetto_amd.WIN_DT, 50, 3, rng), _records(cornetto_amd.IVL_DT, 4000, 3, rng),
            pk, ctg_first)
    return types.SimpleNamespace(held=held, acc=cornetto_amd.Accel, lens_own=lens, gl_ctg=np.array([10, 11, 12]), world=world, rank=rank, lo=3, hi=71)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_format_sample_and_size(tmp_path):
    R = _fake_rank(300_000, 400_000)
    held = R.held
    bench.dump_outputs(R, str(tmp_path / "a"))
    got = _load(tmp_path / "a")
    assert R.held is None                                           # (the step's arrays are let go)
    assert all(a.dtype == np.float64 for a in got.values())
    assert list(got["counts.npy"]) == [300_000, 50, 4000, 400_000] and list(got["cov_thresholds.npy"]) == [3, 71]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in got) <= 64 << 20
    # small arrays whole, in their order, contig ids global
    w = got["telomere_windows.npy"]
    assert w.shape == (50, 4) and "telomere_windows_rows.npy" not in got
    assert np.array_equal(w[:, 0], R.gl_ctg[held[1]["ctg"]]) and np.array_equal(w[:, 1:], np.stack([held[1][c] for c in ("start", "end", "car")], 1))
    # large arrays: DUMP_ROWS rows in their order, their row numbers beside them
    h, rows = got["telomere_runs.npy"], got["telomere_runs_rows.npy"].astype(np.int64)
    assert h.shape == (bench.DUMP_ROWS, 4) and len(np.unique(rows)) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(h[:, 2], held[0]["start"][rows]) and np.array_equal(h[:, 0], R.gl_ctg[held[0]["ctg"][rows]])
    # the packed selection as cornetto_cov_select() rows: (ctg, st, end, depth, mq_depth), end cut at the contig's end
    c, crows = got["selected_cov_windows.npy"], got["selected_cov_windows_rows.npy"].astype(np.int64)
    full = cornetto_amd.Accel.unpack_regs(held[3], held[4], R.lens_own, 2500)
    assert c.shape == (bench.DUMP_ROWS, 5)
    assert np.array_equal(c, np.stack([R.gl_ctg[full["ctg"]]] + [full[k] for k in ("st", "end", "depth", "mq_depth")], 1)[crows])
    # the same records give the same files
    bench.dump_outputs(_fake_rank(300_000, 400_000), str(tmp_path / "b"))
    again = _load(tmp_path / "b")
    assert got.keys() == again.keys() and all(np.array_equal(got[k], again[k]) for k in got)


def test_dump_outputs_of_several_ranks_are_named_by_rank(tmp_path):
    bench.dump_outputs(_fake_rank(300_000, 1000, world=4, rank=2), str(tmp_path))
    got = _load(tmp_path)
    assert all(f.endswith(".rank2.npy") for f in got)
    assert got["telomere_runs.rank2.npy"].shape == (bench.DUMP_ROWS // 4, 4) and got["selected_cov_windows.rank2.npy"].shape == (1000, 5)


def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and p.stdout == b"" and b"--steps" in p.stderr


def _bench(args, timeout=900):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_plain_run_is_lean_and_dumps_what_full_times(tmp_path):
    small = ["--gbases", "0.05", "--steps", "3", "--warmup", "1"]
    plain = _bench(small + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(small + ["--full", "--no-cpu", "--no-profiles", "--no-e2e", "--no-reads", "--emulate-ranks", "", "--dump-outputs", str(tmp_path / "full")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain and k in full
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["unit"] == "Gbases/s" and plain["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in plain]
    assert full["determinism"]["identical"] and "roofline" in full
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert list(a["counts.npy"]) == [plain["results_per_rank"][n] for n in NAMES] == [full["results_per_rank"][n] for n in NAMES]
    assert all(len(a[n + ".npy"]) == min(plain["results_per_rank"][n], bench.DUMP_ROWS) for n in NAMES)
    assert sum(os.path.getsize(tmp_path / "plain" / f) for f in a) <= 64 << 20
