"""bench.py's plain run and --dump-outputs.

CPU: the sample --dump-outputs keeps is fixed and made of whole tiles. GPU: one plain run
(`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`, no --full) prints a line with
the contract's keys and nothing measured beside the timed steps, and the files it writes hold
what the last timed step computed: checked against the oracle on the same capture, at a batch
size above the sampling threshold whose last tile is partial."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from beatrice_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_sample_is_fixed_and_whole_tiles():
    assert np.array_equal(bench.dump_sample(1000), np.arange(1000))
    n = 64 * bench.DUMP_TILES * 3 + 37
    a, b = bench.dump_sample(n), bench.dump_sample(n)
    assert np.array_equal(a, b) and (np.diff(a) > 0).all() and a[-1] < n
    tiles, counts = np.unique(a // 64, return_counts=True)
    assert len(tiles) == bench.DUMP_TILES
    last = (n - 1) // 64
    assert all(c == (37 if t == last else 64) for t, c in zip(tiles, counts))


def test_extra_configs_without_full_are_refused():
    """A plain run measures the headline only: asking it for other configs is an error (before
    anything touches a GPU), not a line that silently lacks them."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--configs", "c3,c4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs --full" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    n = 64 * bench.DUMP_TILES * 2 + 37   # sampled (above DUMP_TILES tiles), last tile partial
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c3", "--packets", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "Mpps" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    # The line rounds ms_per_step and wall_ms to 1e-4 ms and value to 0.01 Mpps, and a step of this
    # batch takes hundredths of a millisecond: the bounds are those rounding quanta, not a
    # relative tolerance. With t the step in ms, |ms - t| <= q, |wall - 3 t| <= q, |value - v| <= 0.005
    # for v = n / t / 1e3, and |n / ms / 1e3 - v| <= (n / ms / 1e3) * q / (ms - q).
    ms, q = d["ms_per_step"], 0.5e-4
    assert ms > 10 * q
    v_ms = n / ms / 1e3
    assert abs(d["value"] - v_ms) <= v_ms * q / (ms - q) + 0.005 + 1e-9
    assert abs(d["timing"]["wall_ms"] - 3 * ms) <= 4 * q + 1e-9
    assert d["timing"]["untimed_prepass_steps"] == 3
    # nothing measured beside the timed steps
    assert d["configs"] == {} and d["roofline"] is None and d["cpu_baseline"] is None
    assert "kernel_pass" not in d["timing"]

    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith(".npy")}
    assert set(got) == {"sample_index", "records", "decide", "verdict", "decide_hist", "verdict_pass", "n_pass",
                        "pass_idx", "pass_idx_sum"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["sample_index"].astype(np.int64)
    assert np.array_equal(idx, bench.dump_sample(n))
    data, desc = synth.capture(synth.C3, n, synth.SEEDS[synth.C3])
    rec, dec, npass = ol.oracle_run(data, desc, n, bench.C3_FILTERS)
    passed = (dec >> 6) == 0
    assert np.array_equal(got["records"], np.ascontiguousarray(rec).view(np.uint8).reshape(n, -1)[idx].view("<u4"))
    assert np.array_equal(got["decide"], dec[idx])
    assert np.array_equal(got["verdict"], passed[idx])
    assert np.array_equal(got["decide_hist"], np.bincount(dec, minlength=256))
    assert got["verdict_pass"][0] == got["n_pass"][0] == npass == passed.sum()
    where = np.nonzero(passed)[0]
    assert np.array_equal(got["pass_idx"], where) and got["pass_idx_sum"][0] == where.sum()
    assert d["config"]["pass_fraction"] == round(npass / n, 4)
