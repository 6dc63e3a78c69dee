"""GPU: two lives of a context, one after the other in one process. Each life compiles a program
with a BT_K_PAYLOAD slot and calls once every part of the runtime that keeps resources on the
context (compaction workspace and compaction stream, DFA pools, host-batch staging, the copy
chunks, the extractor's staging, the timing events, a host registration that is never
unregistered); bt_destroy then has all of it to release. The second life must compute what the
first did, byte for byte, both must equal the goldens / the restatements the calls' own tests
use, and after each destroy the registration the caller left is gone from the process's table.

130 frames: two full 64-frame tiles and a partial one."""
import ctypes
import json
import os

import numpy as np
import pytest

from beatrice_amd import abi, synth
from conftest import GOLDEN, load_golden
from golden_util import compare_decisions
from test_gpu_pass_pack import _reference

pytestmark = pytest.mark.gpu

N = 130
LEAD = 16
TABLE = "parser_example"


def _pins():
    buf = (ctypes.c_uint64 * (3 * 64))()
    n = ctypes.c_uint32(0)
    abi._check(abi.lib().bt_host_pins(buf, 64, ctypes.byref(n)))
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(min(n.value, 64))]


def _overlapping(arr):
    lo, hi = arr.ctypes.data, arr.ctypes.data + arr.nbytes
    return [p for p in _pins() if p[0] < hi and lo < p[1]]


def _life(g, filters, ex, table):
    """One context from bt_create to bt_destroy; returns (every output by name, the array left
    registered)."""
    data, desc = g["data"], g["desc"][:N]
    out = {}
    left = abi.host_array(2 * abi.PAGE)
    ctx = abi.Context(0, host_chunk_packets=4096)
    try:
        kinds = [abi.KINDS[s.kind] for s in ctx.compile(filters)]
        assert "PAYLOAD" in kinds and "HOST" not in kinds, kinds

        # device-resident: records + decisions + verdict words + pass list
        run = abi.DeviceRun(ctx, data, desc, N)
        run.run()
        out.update({f"device.{k}": v for k, v in run.fetch().items()})
        # the same with the compaction on the context's own stream
        for b in (run.d_rec, run.d_dec, run.d_ver, run.d_pidx, run.d_npass):
            b.zero()
        ctx.run_device_async(run.batch, run.outs)
        out.update({f"async.{k}": v for k, v in run.fetch().items()})
        # ... and twice from the timed loop
        for b in (run.d_rec, run.d_dec, run.d_ver, run.d_pidx, run.d_npass):
            b.zero()
        ctx.time_device(run.batch, run.outs, 2)
        out.update({f"timed.{k}": v for k, v in run.fetch().items()})

        # the ordered pack of the passing frames, each behind 16 bytes of what precedes it
        sel = (out["device.decide"] >> 6) == abi.DECIDE_PASS
        off, ln = synth.desc_off(desc).astype(np.int64), synth.desc_len(desc).astype(np.int64)
        cap = int((LEAD + ln[sel]).sum())
        d_out, d_odesc, d_tot = ctx.alloc(cap + 64), ctx.alloc(N * 8), ctx.alloc(16)
        ctx.pass_pack(run.batch, run.d_ver, d_out, cap, d_tot.ptr, d_tot.ptr + 8, desc=d_odesc, lead=LEAD)
        ctx.synchronize()
        tot = d_tot.download(np.zeros(16, np.uint8))
        out["pack.total"], out["pack.n_packed"] = tot[:8].view(np.uint64).copy(), tot[8:12].view(np.uint32).copy()
        out["pack.bytes"] = d_out.download(np.zeros(cap + 64, np.uint8))[:cap]
        out["pack.desc"] = d_odesc.download(np.zeros(N, np.uint64))[:int(sel.sum())]
        for b in (d_out, d_odesc, d_tot):
            b.free()
        run.free()

        # a prefix batch, then the resume pass over the whole frames
        two = abi.DeviceRun(ctx, data, desc, N, records=False)
        two.batch.flags = abi.BATCH_PREFIXES
        two.run()
        out["prefix.decide"] = two.fetch()["decide"].copy()
        two.batch.flags = 0
        two.d_ver.upload(np.full(two.d_ver.nbytes, 0xA5, np.uint8))
        ctx.resume_device(two.batch, two.outs)
        out.update({f"resume.{k}": v for k, v in two.fetch().items()})
        two.free()

        # a host batch with records
        out.update({f"host.{k}": np.copy(v) for k, v in ctx.run_host(data, desc).items() if k != "n_pass"})

        # bt_memcpy_h2d / bt_memcpy_d2h, a buffer longer than one of the context's copy chunks
        blob = np.random.default_rng(5).integers(0, 256, (8 << 20) + 4133, dtype=np.uint8)
        d_blob = ctx.alloc(blob.nbytes)
        d_blob.upload(blob)
        out["copy.back"] = d_blob.download(np.zeros(blob.nbytes, np.uint8))
        d_blob.free()
        assert np.array_equal(out["copy.back"], blob)

        # the extractor over host lists
        eoff, eln = synth.desc_off(ex["desc"][:N]), synth.desc_len(ex["desc"][:N])
        frames = [ex["data"][o:o + m].tobytes() for o, m in zip(eoff, eln)]
        out["extract.status"], out["extract.values"], out["extract.image"] = ctx.extract_host(frames, table)

        # a registration the caller never takes back
        ctx.register(left)
        assert _overlapping(left), "the registered range is not in the table"
    finally:
        ctx.close()
    return out, left


def _check(out, g, filters, ex, table):
    data, desc = g["data"], g["desc"][:N]
    code, src = g["code__payload_chain"][:N], g["src__payload_chain"][:N]
    want = code == 0
    assert 0 < want.sum() < N
    for call in ("device", "async", "timed", "resume", "host"):
        dec = out[f"{call}.decide"]
        assert not ((dec >> 6) == abi.DECIDE_HOST).any(), call
        compare_decisions(dec, code, src, filters, where=call)
        bits = np.unpackbits(out[f"{call}.verdict"].view(np.uint8), bitorder="little")
        assert np.array_equal(bits[:N].astype(bool), want) and not bits[N:].any(), call
        assert np.array_equal(out[f"{call}.pass_idx"], np.nonzero(want)[0]), call
        if call != "host":
            assert out[f"{call}.n_pass"] == int(want.sum()), call
    for call in ("device", "async", "timed", "host"):
        assert np.array_equal(out[f"{call}.records"], g["rec"][:N]), f"{call}: records differ from the reference fixture"
    first = out["prefix.decide"]
    assert ((first >> 6) == abi.DECIDE_HOST).any(), "the prefix pass left no work"

    off, ln = synth.desc_off(desc).astype(np.int64), synth.desc_len(desc).astype(np.int64)
    cap = int((LEAD + ln[want]).sum())
    body, pdesc, total, n_packed = _reference(data, len(data), off, ln, want, LEAD, 0, 1, cap)
    assert int(out["pack.total"][0]) == total == cap and int(out["pack.n_packed"][0]) == n_packed == int(want.sum())
    assert np.array_equal(out["pack.bytes"], body) and np.array_equal(out["pack.desc"], pdesc)

    assert np.array_equal(out["extract.status"], ex[f"status__{TABLE}"][:N])
    assert np.array_equal(out["extract.values"], ex[f"values__{TABLE}"][:, :N])
    span = out["extract.image"].shape[1]
    ok = out["extract.status"] == 0
    eoff = synth.desc_off(ex["desc"][:N])
    for i in np.nonzero(ok)[0]:
        assert np.array_equal(out["extract.image"][i], ex["data"][eoff[i]:eoff[i] + span])
    assert 0 < ok.sum() and not out["extract.image"][~ok].any()


def test_two_context_lifetimes():
    g, man = load_golden("http")
    filters = man["filter_sets"]["payload_chain"]
    with open(os.path.join(GOLDEN, "extract.json")) as fh:
        table = json.load(fh)["tables"][TABLE]
    ex = dict(np.load(os.path.join(GOLDEN, "extract.npz"), allow_pickle=False))
    lives = []
    for k in range(2):
        out, left = _life(g, filters, ex, table)
        assert not _overlapping(left), f"life {k}: the range left registered outlived its context"
        _check(out, g, filters, ex, table)
        lives.append(out)
    assert lives[0].keys() == lives[1].keys()
    for name in lives[0]:
        a, b = np.asarray(lives[0][name]), np.asarray(lives[1][name])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: life 2 differs from life 1"
