"""GPU: oracle/_ref/test_device_stats (tests/cpp/test_device_stats.cpp), GpuPacketFilter::
classifyDevice beside the compiled reference PacketFilter on the golden captures: the statistics
of a batch that stays on the device (getStats(): processed / passed / dropped and the whole
filterCounts map) and the exception of a throwing expression equal the reference's
applyFilters(vector), for the sets c3, mixed, empty, throw_after and throw_oor; a second call
accumulates, resetStats starts over, a CUSTOM callback is refused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "test_device_stats")


@pytest.mark.parametrize("cap", ["edge", "fuzz"])
def test_classify_device_matches_the_reference_stats(cap, tmp_path):
    assert os.path.exists(BIN), "oracle/_ref/test_device_stats is not built (make -C oracle ref)"
    g, _ = load_golden(cap)
    desc = np.ascontiguousarray(g["desc"], dtype=np.uint64)
    data = np.ascontiguousarray(g["data"], dtype=np.uint8)
    path = tmp_path / f"{cap}.bin"
    with open(path, "wb") as fh:
        fh.write(np.uint64(len(desc)).tobytes())
        fh.write(desc.tobytes())
        fh.write(np.uint64(data.nbytes).tobytes())
        fh.write(data.tobytes())
    r = subprocess.run([BIN, str(path), cap], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    for fset in ("c3", "mixed", "empty", "throw_after", "throw_oor"):
        assert f"ok {cap}/{fset}:" in r.stdout
