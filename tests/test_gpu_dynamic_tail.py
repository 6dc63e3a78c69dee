"""The dynamic tail of the late-issue main kernel (64-B fixed stride with a filter;
beatrice_amd/csrc/bt_tail_split.h) against the oracle, the way test_blocked_tile_ranges checks the
blocked order: C2 frames at stride 64 with C3's three filters on 8 waves, so that small batches
run every phase of the deal — a single tile, fewer tiles than waves, a tail that is the whole
batch, a static part and a tail with the partial last tile inside the tail, an exact multiple.
Records, decisions, verdict words, the pass list and n_pass are compared bit for bit; the 101-tile
batch also with one output requested at a time, three times on one context, and as four pipelined
steps over two output sets (the counters' reuse from launch to launch)."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from beatrice_amd import abi, synth

pytestmark = pytest.mark.gpu

FILTERS = [{"type": abi.PROTOCOL, "expr": "udp", "priority": 3},
           {"type": abi.IP_RANGE, "expr": "10.0.0.0/8", "priority": 2},
           {"type": abi.PORT_RANGE, "expr": "1000-2000", "priority": 1}]
N_ALL = 6405          # 101 tiles, the last one partial
SIZES = {63: 1, 448: 7, 1541: 25, 6405: 101, 6400: 100}   # n: tiles


@functools.lru_cache(maxsize=None)
def frames():
    data, _ = synth.capture(synth.C2, N_ALL, seed=0x7A11)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def reference(n):
    """(records, decisions, verdict words, pass list) of the first n frames, from the oracle."""
    rec, dec, npass = ol.oracle_run(np.ascontiguousarray(frames()[:n * 64]), None, n, FILTERS, stride=64)
    passing = np.nonzero((dec >> 6) == 0)[0].astype(np.uint32)
    assert len(passing) == npass
    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
    bits[passing] = 1
    words = np.packbits(bits, bitorder="little").view(np.uint64)
    for a in (rec, dec, words, passing):
        a.setflags(write=False)
    return rec, dec, words, passing


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0, grid_waves=8)
    c.compile(FILTERS)
    yield c
    c.close()


def device_run(ctx, n, **outs):
    return abi.DeviceRun(ctx, np.ascontiguousarray(frames()[:n * 64]), None, n, stride=64, **outs)


def check(out, n, what):
    rec, dec, words, passing = reference(n)
    if "records" in out:
        assert np.array_equal(out["records"], rec), f"{what}: records"
    if "decide" in out:
        assert np.array_equal(out["decide"], dec), f"{what}: decisions"
    if "verdict" in out:
        assert np.array_equal(out["verdict"], words), f"{what}: verdict words"
    if "pass_idx" in out:
        assert out["n_pass"] == len(passing), f"{what}: n_pass"
        assert np.array_equal(out["pass_idx"], passing), f"{what}: pass list"


@pytest.mark.parametrize("n", list(SIZES))
def test_every_phase_of_the_deal(ctx, n):
    assert (n + 63) // 64 == SIZES[n]
    r = device_run(ctx, n)
    try:
        r.run()
        check(r.fetch(), n, f"n={n}")
    finally:
        r.free()


@pytest.mark.parametrize("only", ["decide", "verdict", "pass_idx", "records"])
def test_one_output_at_a_time(ctx, only):
    """Only the decisions, only the verdict words, only the pass list (the empty buffer ranges of
    the counted stores), and records only (the parse-only kernel: static deal)."""
    want = dict(records=False, decide=False, verdict=False, pass_idx=False)
    want[only] = True
    r = device_run(ctx, N_ALL, **want)
    try:
        r.run()
        out = r.fetch()
        assert only in out
        check(out, N_ALL, f"{only} alone")
    finally:
        r.free()


def test_counters_are_reused_across_launches(ctx):
    """Three launches on one context, then four pipelined steps over two output sets: every
    launch finds the counters its predecessor left and must deal every tile once again."""
    r = device_run(ctx, N_ALL)
    alt = device_run(ctx, N_ALL)
    try:
        for i in range(3):
            for buf in (r.d_rec, r.d_dec, r.d_ver, r.d_pidx, r.d_npass):
                buf.zero()
            r.run()
            check(r.fetch(), N_ALL, f"launch {i}")
        for s in (r, alt):
            for buf in (s.d_rec, s.d_dec, s.d_ver, s.d_pidx, s.d_npass):
                buf.zero()
        ctx.synchronize()
        for i in range(4):
            ctx.run_device_async(r.batch, (r, alt)[i % 2].outs)
            if i == 1:   # the first two steps' outputs, before steps 2 and 3 rewrite them
                check(r.fetch(), N_ALL, "pipelined step 0")
                check(alt.fetch(), N_ALL, "pipelined step 1")
                for s in (r, alt):
                    for buf in (s.d_rec, s.d_dec, s.d_ver, s.d_pidx, s.d_npass):
                        buf.zero()
                ctx.synchronize()
        check(r.fetch(), N_ALL, "pipelined step 2")
        check(alt.fetch(), N_ALL, "pipelined step 3")
    finally:
        r.free()
        alt.free()


def test_a_block_of_every_label():
    """64 waves (16 blocks: every head has blocks of its own label, so a wave tries only the first
    few heads): 391 tiles are two static rounds and a tail of 263 tiles, the last one partial."""
    n = 25003
    data, _ = synth.capture(synth.C2, n, seed=0x7A12)
    rec, dec, npass = ol.oracle_run(data, None, n, FILTERS, stride=64)
    c = abi.Context(0, grid_waves=64)
    try:
        c.compile(FILTERS)
        r = abi.DeviceRun(c, data, None, n, stride=64)
        for i in range(2):
            r.run()
            out = r.fetch()
            assert np.array_equal(out["records"], rec), f"launch {i}: records"
            assert np.array_equal(out["decide"], dec), f"launch {i}: decisions"
            assert out["n_pass"] == npass, f"launch {i}: n_pass"
            assert np.array_equal(out["pass_idx"], np.nonzero((dec >> 6) == 0)[0]), f"launch {i}: pass list"
            bits = np.unpackbits(out["verdict"].view(np.uint8), bitorder="little")[:n]
            assert np.array_equal(bits, (dec >> 6) == 0), f"launch {i}: verdict words"
        r.free()
    finally:
        c.close()


def test_a_callers_stream_has_its_own_counters(ctx):
    """The same batch on a caller's stream and on the context's, queued back to back."""
    r = device_run(ctx, N_ALL)
    alt = device_run(ctx, N_ALL)
    st = ctx.stream_create()
    try:
        ctx.run_device(r.batch, r.outs, stream=st)
        ctx.run_device(alt.batch, alt.outs)
        ctx.stream_synchronize(st)
        check(r.fetch(), N_ALL, "caller's stream")
        check(alt.fetch(), N_ALL, "context stream")
    finally:
        ctx.stream_destroy(st)
        r.free()
        alt.free()
