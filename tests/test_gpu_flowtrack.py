"""GPU: the flow tracker (bt_flow_track_*_device, beatrice_amd/csrc/bt_flowtrack.hip): a flow table
that lives across batches on the device. Expected values come from the restatement in
flowtrack_ref.py (a dict over (class, key bytes) that lives across batches), never from the code
under test; the host form must agree bit for bit. Every state, scratch and output sits in a
poisoned buffer between two 256-byte guards. A sequence's buffers are allocated, poisoned and
uploaded first; then its calls are enqueued back to back and waited for once."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import POISON, STRIDE, Guarded, Source, golden_keys, select_words, strided  # noqa: E402

pytestmark = pytest.mark.gpu

BT_E_INVALID_ARGUMENT = 1


class DevTracker:
    """A tracker state on the device, the restatement and the host form side by side. update() and
    expire() prepare a call (its guarded buffers, its uploads, what it must give); finish() enqueues the
    init and every prepared call back to back, waits once and compares everything."""

    def __init__(self, ctx, flow_cap, flags=0, slots=0, stream=None):
        self.ctx, self.flow_cap, self.flags, self.stream = ctx, flow_cap, flags, stream
        self.layout = abi.flow_track_layout(flow_cap, slots)
        self.state = Guarded(ctx, self.layout["total"])
        self.ref = fkr.Tracker(flow_cap, flags, slots)
        self.host = abi.HostFlowTracker(flow_cap, flags, slots)
        self.pending, self.keep, self.slots, self.started = [], [], slots, False

    def update(self, batch, n, keys, lens, host_data=None, host_desc=None, select=None, ts=None, batch_ts=0, want_ids=True, where=""):
        """keys: flow_ref's (inputs, nbytes, klass) of the batch's n packets. host_data / host_desc: the same
        batch for the host form (packed descriptors), when there is one."""
        ctx = self.ctx
        need = abi.flow_track_scratch_bytes(n)
        bufs = {"flow_id": Guarded(ctx, 4 * n) if want_ids else None, "result": Guarded(ctx, 64), "scratch": Guarded(ctx, need)}
        d_sel = d_ts = None
        if select is not None:
            d_sel = ctx.alloc(max(16, select.nbytes))
            d_sel.upload(select)
        if ts is not None and n:
            d_ts = ctx.alloc(8 * n)
            d_ts.upload(np.asarray(ts, np.uint64))
        def call():
            ctx.flow_track_update(self.state.ptr, batch, bufs["scratch"].ptr, need, bufs["result"].ptr, select=d_sel,
                                  ts=d_ts, batch_ts=batch_ts, flow_id=bufs["flow_id"].ptr if want_ids else None, stream=self.stream)
        t = ts if n else None
        want = self.ref.update(keys[0], keys[1], keys[2], lens, select, t, batch_ts)
        host = None
        if host_desc is None:
            self.host = None   # a batch the host form does not take (fixed stride, XDP descriptors as such)
        elif self.host is not None:
            host = self.host.update(host_data, host_desc, select, t, batch_ts)
        self.pending.append(("update", where, bufs, want, host, call))
        self.keep += [d_sel, d_ts]

    def expire(self, now, idle, expired_cap=None, where=""):
        ctx = self.ctx
        need = abi.flow_track_expire_scratch_bytes(self.flow_cap)
        bufs = {"expired": Guarded(ctx, 104 * expired_cap) if expired_cap is not None else None, "remap": Guarded(ctx, 4 * self.flow_cap),
                "result": Guarded(ctx, 32), "scratch": Guarded(ctx, need)}
        def call():
            ctx.flow_track_expire(self.state.ptr, now, idle, bufs["scratch"].ptr, need, bufs["result"].ptr,
                                  expired=bufs["expired"].ptr if bufs["expired"] else None, expired_cap=expired_cap or 0,
                                  remap=bufs["remap"].ptr, stream=self.stream)
        want = self.ref.expire(now, idle, expired_cap)
        host = self.host.expire(now, idle, expired_cap) if self.host is not None else None
        self.pending.append(("expire", where, bufs, want, host, call))

    def finish(self, host_too=True):
        """The one wait; every call's outputs against the restatement (and the host form's), then the
        state: header and the whole record region. Returns the state's header and record bytes."""
        ctx = self.ctx
        ctx.synchronize()   # the uploads and the poison are in place
        if not self.started:
            ctx.flow_track_init(self.state.ptr, self.layout["total"], self.flow_cap, self.flags, self.slots, stream=self.stream)
            self.started = True
        for item in self.pending:   # nothing but the calls themselves from here to the wait
            item[5]()
        if self.stream is not None:
            ctx.stream_synchronize(self.stream)
        ctx.synchronize()
        for kind, where, bufs, want, host, _ in self.pending:
            bufs["scratch"].read()   # its guards
            if kind == "update":
                res = abi.FlowTrackResult.from_bytes(bufs["result"].read()).as_dict()
                assert res == want["result"], f"{where}: result " + ", ".join(k for k in res if res[k] != want["result"][k])
                if bufs["flow_id"] is not None:
                    fid = bufs["flow_id"].read(np.uint32)
                    bad = np.nonzero(fid != want["flow_id"])[0]
                    assert len(bad) == 0, f"{where}: flow_id differs at {bad[:8]}: {fid[bad[:8]]} != {want['flow_id'][bad[:8]]}"
                    if host is not None:
                        assert (host[0] == fid).all(), f"{where}: the host form's flow_id"
                if host is not None:
                    assert host[1] == res, f"{where}: the host form's result"
            else:
                res = abi.FlowTrackExpireResult.from_bytes(bufs["result"].read()).as_dict()
                assert res == want["result"], f"{where}: expire result {res} != {want['result']}"
                remap = bufs["remap"].read(np.uint32)
                nb = res["n_flows_before"]
                assert (remap[:nb] == want["remap"]).all(), f"{where}: remap"
                assert (remap[nb:] == np.uint32(0x01010101 * POISON)).all(), f"{where}: remap written at or past n_flows_before"
                assert host is None or ((host[1][:nb] == remap[:nb]).all() and host[2] == res)
                if bufs["expired"] is not None:
                    exp = bufs["expired"].read()
                    ne = res["n_expired"]
                    assert exp[:104 * ne].tobytes() == want["expired"].tobytes(), f"{where}: expired records"
                    assert host is None or host[0].tobytes() == want["expired"].tobytes(), f"{where}: the host form's expired records"
                    assert (exp[104 * ne:] == POISON).all(), f"{where}: expired written at or past n_expired"
            for b in bufs.values():
                if b is not None:
                    b.free()
        self.pending = []
        for b in self.keep:
            if b is not None:
                b.free()
        self.keep = []
        raw = self.state.read()
        lay = self.layout
        hdr = abi.FlowTrackHdr.from_bytes(raw).as_dict()
        want = self.ref.header()
        assert hdr == want, "header " + ", ".join(k for k in hdr if hdr[k] != want[k])
        recs = raw[lay["records"]:lay["records"] + 104 * self.flow_cap]
        assert recs.tobytes() == self.ref.records(whole=True).tobytes(), "records"
        assert (raw[128:lay["records"]] == POISON).all() and (raw[lay["records"] + 104 * self.flow_cap:lay["slot_words"]] == POISON).all()
        if host_too and self.host is not None:   # bit for bit: header and records (the slot words are private to each side)
            assert self.host.state[:128].tobytes() == raw[:128].tobytes()
            assert self.host.state[lay["records"]:lay["records"] + 104 * self.flow_cap].tobytes() == recs.tobytes()
        return raw[:128].tobytes(), recs.tobytes()

    def free(self):
        if self.started:
            abi.Context.flow_track_forget(self.state.ptr)   # before the memory goes back
        self.state.free()


# name, format, flags, selection, flow_cap (None: room for all), per batch (n, first frame of the golden)
SEQUENCES = [
    ("c3", "packed", 0, "null", None, [(63, 0), (64, 40), (16384, 100), (0, 0)]),
    ("fuzz", "xdp", ftr.BIDIRECTIONAL, "random", None, [(65, 0), (1, 30), (16385, 50), (64, 8000)]),
    ("c4", "packed", ftr.L3_ONLY | ftr.BIDIRECTIONAL, "null", 1000, [(16385, 0), (0, 0), (65, 2000), (16384, 1000)]),
    ("edge", "packed", ftr.L3_ONLY, "random", 5, [(1, 5), (63, 0), (65, 100), (16385, 7)]),   # 8 flows by address
]


def run_sequence(ctx, seq, stream=None, per_packet_ts=True):
    """Four batches of a golden, shifted so that some flows recur and some are new; one expire; one
    more batch, which must find the flows that stayed. Returns the final (header, records) bytes."""
    name, fmt, flags, kind, cap, batches = seq
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    inputs, nbytes, klass = golden_keys(name, bool(flags & ftr.L3_ONLY))
    cap = cap or n0
    t = DevTracker(ctx, cap, flags, stream=stream)
    rng = np.random.default_rng(n0 + flags)
    srcs = []
    try:
        for b, (n, start) in enumerate(batches + [(65, 10)]):
            if b == len(batches):   # flows with a last packet before 500 leave, in two calls when there is no room for all
                t.expire(1000, 500, expired_cap=7 if kind == "random" else None, where=f"{name} expire")
            reps = (start + np.arange(n)) % n0
            desc = g["desc"][reps]
            src = Source(ctx, name, n, fmt, desc=desc)   # the golden's data, these descriptors
            srcs.append(src)
            sel = select_words(kind, n, seed=b)
            ts = rng.integers(0, 1000, n).astype(np.uint64) if per_packet_ts else None
            t.update(src.batch, n, (inputs[reps], nbytes[reps], klass[reps]), src.lens, g["data"], desc, sel, ts,
                     batch_ts=100 * b, want_ids=b != 1, where=f"{name} {fmt} batch {b} n={n}")
        out = t.finish()
        assert t.ref.seq == len(batches) + 1
        return out, t.ref
    finally:
        t.free()
        for s in srcs:
            s.free()


@pytest.mark.parametrize("seq", SEQUENCES, ids=[s[0] for s in SEQUENCES])
def test_sequences_of_batches_then_expire_then_find_again(gpu_ctx, seq):
    st = gpu_ctx.stream_create()
    try:
        first, ref = run_sequence(gpu_ctx, seq, stream=st)
        second, _ = run_sequence(gpu_ctx, seq)   # another state, the context's stream: identical header and records
        assert first == second
    finally:
        gpu_ctx.stream_destroy(st)
    h = ref.header()
    assert h["n_flows"] > 0 and h["seq"] == 5
    if seq[4]:
        assert h["overflow_packets"] > 0   # the cap was met


def test_fixed_stride_and_scalar_timestamps(gpu_ctx):
    """Fixed-stride frames (the keys from the Python walk over the cut frames) and batch_ts instead of ts[]."""
    name, flags = "fuzz", ftr.BIDIRECTIONAL
    _, keys = strided(name)
    inputs, nbytes, klass = keys[False]
    t = DevTracker(gpu_ctx, 4000, flags)
    srcs = []
    try:
        for b, n in enumerate((65, 16385, 64)):
            src = Source(gpu_ctx, name, n, "stride")
            srcs.append(src)
            r = src.reps
            sel = select_words("random", n, seed=b)
            t.update(src.batch, n, (inputs[r], nbytes[r], klass[r]), src.lens, None, None, sel, None, batch_ts=10 + b,
                     where=f"stride batch {b}")
        t.expire(12, 0, expired_cap=4000, where="stride expire")   # the flows last seen in batch 0 or 1
        t.finish(host_too=False)
        assert 0 < t.ref.header()["n_flows"] and (t.ref.records()["last_ts"] == 12).all()
    finally:
        t.free()
        for s in srcs:
            s.free()


def _frame64(k):
    """A 64-byte IPv4 / TCP frame of flow k."""
    ip = bytes([0x45, 0, 0, 50, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes([10, 1, k >> 16 & 255, k >> 8 & 255]) + bytes([10, 2, 0, k & 255])
    return bytes(12) + b"\x08\x00" + ip + (1024 + (k & 0x7FFF)).to_bytes(2, "big") + (443).to_bytes(2, "big") + bytes(26)


def _stride64(ctx, ks):
    frames = [_frame64(k) for k in ks]
    assert all(len(f) == 64 for f in frames)
    host = np.frombuffer(b"".join(frames), np.uint8)
    d = ctx.alloc(max(256, len(host)))
    d.upload(host)
    keys = fr.key_of_frames(frames)
    return d, abi.Batch(d.ptr, None, 64, len(frames), 0, 0, 0), keys


def test_every_packet_its_own_flow_at_16385(gpu_ctx):
    n = 16385
    d, batch, keys = _stride64(gpu_ctx, range(n))
    t = DevTracker(gpu_ctx, n)
    try:
        t.update(batch, n, keys, np.full(n, 64), batch_ts=5, where="16385 new flows")
        t.update(batch, n, keys, np.full(n, 64), batch_ts=6, where="16385 found flows")
        hdr, _ = t.finish(host_too=False)
        assert t.ref.header()["n_flows"] == n and (t.ref.records()["packets"][:, 0] == 2).all()
    finally:
        t.free()
        d.free()


def test_a_table_loaded_to_one(gpu_ctx):
    """128 flows into flow_cap = slots = 128 fill every slot; a 129th flow overflows; the same 128 keys again are all found."""
    d0, b0, k0 = _stride64(gpu_ctx, range(128))
    d1, b1, k1 = _stride64(gpu_ctx, [128, 5, 128])
    d2, b2, k2 = _stride64(gpu_ctx, list(reversed(range(128))))
    t = DevTracker(gpu_ctx, 128, slots=128)
    try:
        t.update(b0, 128, k0, np.full(128, 64), batch_ts=1, where="128 flows")
        t.update(b1, 3, k1, np.full(3, 64), batch_ts=2, where="the 129th")
        t.update(b2, 128, k2, np.full(128, 64), batch_ts=3, where="the 128 again")
        t.finish(host_too=False)
        h = t.ref.header()
        assert (h["n_flows"], h["overflow_packets"], h["overflow_bytes"]) == (128, 2, 128)
        slots = t.state.read(np.uint32)[t.layout["slot_words"] // 4:]
        assert len(slots) == 128 and sorted(slots.tolist()) == list(range(128))   # every slot holds a flow, each flow once
    finally:
        t.free()
        for d in (d0, d1, d2):
            d.free()


def test_a_state_that_is_not_this_tracker_is_left_alone(gpu_ctx):
    """The refusals that need an initialised state, and the kernels' own check of the header."""
    L = abi.lib()
    d, batch, keys = _stride64(gpu_ctx, range(10))
    t = DevTracker(gpu_ctx, 64)
    res, scratch, ids = Guarded(gpu_ctx, 64), Guarded(gpu_ctx, abi.flow_track_scratch_bytes(10)), Guarded(gpu_ctx, 40)
    xres, xscratch = Guarded(gpu_ctx, 32), Guarded(gpu_ctx, abi.flow_track_expire_scratch_bytes(64))
    try:
        t.finish(host_too=False)   # the init alone: an empty tracker
        upd, out = abi.FlowTrackUpdate(None, 0), abi.FlowTrackOut(None, res.ptr)
        rc = L.bt_flow_track_update_device(None, t.state.ptr, ctypes.byref(batch), None, ctypes.byref(upd), scratch.ptr, scratch.size,
                                           ctypes.byref(out), None)
        assert rc == BT_E_INVALID_ARGUMENT and "null context" in L.bt_last_error().decode()
        xout = abi.FlowTrackExpireOut(None, 0, 0, None, xres.ptr)
        rc = L.bt_flow_track_expire_device(None, t.state.ptr, 1, 1, xscratch.ptr, xscratch.size - 256, ctypes.byref(xout), None)
        assert rc == BT_E_INVALID_ARGUMENT and "below the need" in L.bt_last_error().decode()
        rc = L.bt_flow_track_expire_device(None, t.state.ptr, 1, 1, xscratch.ptr, xscratch.size, ctypes.byref(xout), None)
        assert rc == BT_E_INVALID_ARGUMENT and "null context" in L.bt_last_error().decode()
        # the header overwritten behind the library's back: both calls change nothing and say so
        abi._check(L.bt_memset_d(gpu_ctx.h, t.state.ptr, 0, 128))
        gpu_ctx.flow_track_update(t.state.ptr, batch, scratch.ptr, scratch.size, res.ptr, flow_id=ids.ptr)
        gpu_ctx.flow_track_expire(t.state.ptr, 1, 1, xscratch.ptr, xscratch.size, xres.ptr)
        gpu_ctx.synchronize()
        r = abi.FlowTrackResult.from_bytes(res.read()).as_dict()
        assert r == {**dict.fromkeys(r, 0), "n": 10, "status": 1}
        assert (ids.read(np.uint32) == abi.FLOW_ID_UNSELECTED).all()   # no per-batch number is left to pass for a flow number
        x = abi.FlowTrackExpireResult.from_bytes(xres.read()).as_dict()
        assert x["status"] == 1 and x["n_expired"] == 0
        raw = t.state.read()
        lay = t.layout
        assert (raw[:128] == 0).all() and (raw[lay["records"]:lay["records"] + 104 * 64] == 0).all()
        assert (raw[lay["slot_words"]:] == 0xFF).all()
        scratch.read()
        xscratch.read()
    finally:
        t.free()
        d.free()
        for b in (res, scratch, xres, xscratch, ids):
            b.free()


def test_the_library_knows_256_states_and_drops_none(gpu_ctx):
    """The 257th address is refused with its reason and launches nothing; forgetting one makes room;
    a forgotten state is refused by the later calls."""
    L = abi.lib()
    size = abi.flow_track_layout(1)["total"]
    pool = gpu_ctx.alloc(300 * size)
    abi._check(L.bt_memset_d(gpu_ctx.h, pool.ptr, 0x5A, pool.nbytes))
    opts = abi.FlowTrackOpts(0, 1, 0, 0)
    known = []
    try:
        for k in range(300):
            rc = L.bt_flow_track_init_device(gpu_ctx.h, pool.ptr + k * size, size, ctypes.byref(opts), None)
            if rc:
                break
            known.append(pool.ptr + k * size)
        assert rc == 3 and "256 tracker states" in L.bt_last_error().decode() and 0 < len(known) <= 256   # BT_E_RESOURCE
        gpu_ctx.synchronize()
        refused = pool.download(np.zeros(pool.nbytes, np.uint8))[len(known) * size:(len(known) + 1) * size]
        assert (refused == 0x5A).all()
        assert L.bt_flow_track_init_device(gpu_ctx.h, known[0], size, ctypes.byref(opts), None) == 0   # a known address again
        gpu_ctx.flow_track_forget(known[3])
        assert L.bt_flow_track_forget(known[3]) == BT_E_INVALID_ARGUMENT and "not an initialised tracker" in L.bt_last_error().decode()
        assert L.bt_flow_track_forget(None) == BT_E_INVALID_ARGUMENT
        xres, xscratch = gpu_ctx.alloc(32), gpu_ctx.alloc(abi.flow_track_expire_scratch_bytes(1))
        xout = abi.FlowTrackExpireOut(None, 0, 0, None, xres.ptr)
        rc = L.bt_flow_track_expire_device(gpu_ctx.h, known[3], 1, 1, xscratch.ptr, xscratch.nbytes, ctypes.byref(xout), None)
        assert rc == BT_E_INVALID_ARGUMENT and "not an initialised tracker" in L.bt_last_error().decode()
        assert L.bt_flow_track_init_device(gpu_ctx.h, pool.ptr + len(known) * size, size, ctypes.byref(opts), None) == 0
        known[3] = pool.ptr + len(known) * size
        gpu_ctx.synchronize()
        xres.free()
        xscratch.free()
    finally:
        for s in known:
            L.bt_flow_track_forget(s)
        pool.free()
