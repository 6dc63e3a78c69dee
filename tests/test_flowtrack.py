"""CPU: the flow tracker on the host (bt_flow_track_init_host / _update_host / _expire_host,
include/beatrice_gpu.h) against the restatement in flowtrack_ref.py (a dict over (class, key bytes)
that lives across batches, built on flowtab_ref.py and flow_ref.py), the layout and scratch sizes,
the ctypes layout of the new structs, and the refusals of the device calls, which need no GPU."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
import flowtab_ref as ftr
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)


@functools.lru_cache(maxsize=None)
def golden_keys(name, l3_only=False):
    g, _ = load_golden(name)
    return fr.key_of_rec(g["rec"], l3_only)


def random_select(n, rng):
    """Verdict-layout words with garbage in the bits at or above n."""
    if n == 0:
        return None
    w = fr.pack_bits(rng.integers(0, 2, n).astype(bool))
    if n % 64:
        w[-1] |= ~np.uint64(0) << np.uint64(n % 64)
    return w


def same_state(host, ref, where=""):
    """Header and the whole record region of a HostFlowTracker against the restatement."""
    got, want = host.header(), ref.header()
    assert got == want, f"{where}: header " + ", ".join(k for k in got if got[k] != want[k])
    lay = host.layout
    recs = host.state[lay["records"]:lay["records"] + 104 * host.flow_cap]
    assert recs.tobytes() == ref.records(whole=True).tobytes(), f"{where}: records"


def run_golden(name, reps_n, cuts, flags, selected, flow_cap=None):
    """The golden's frames (repeated up to reps_n) in `cuts` batches through the host tracker and
    the restatement, every flow_id and result compared. Returns (host, ref, bounds, selection bits)."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    desc, reps = np.resize(g["desc"], reps_n), np.resize(np.arange(n0), reps_n)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    inputs, nbytes, klass = golden_keys(name, bool(flags & ftr.L3_ONLY))
    bounds = np.linspace(0, reps_n, cuts + 1).astype(int)
    cap = reps_n if flow_cap is None else flow_cap
    host, ref = abi.HostFlowTracker(cap, flags), fkr.Tracker(cap, flags)
    rng = np.random.default_rng(reps_n + cuts + flags)
    bits = []
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        sel = random_select(hi - lo, rng) if selected else None
        ts = rng.integers(0, 1 << 40, hi - lo).astype(np.uint64)   # not monotonic: last_ts is the last packet's, not the maximum
        bits.append(fr.select_bits(sel, hi - lo))
        r = reps[lo:hi]
        fid, res = host.update(g["data"], desc[lo:hi], sel, ts)
        want = ref.update(inputs[r], nbytes[r], klass[r], lens[lo:hi], sel, ts)
        where = f"{name} batch {b}/{cuts} flags={flags}"
        assert res == want["result"], f"{where}: result " + ", ".join(k for k in res if res[k] != want["result"][k])
        assert (fid == want["flow_id"]).all(), f"{where}: flow_id at {np.nonzero(fid != want['flow_id'])[0][:8]}"
    same_state(host, ref, f"{name} x{cuts} flags={flags}")
    return host, ref, bounds, np.concatenate(bits) if bits else np.zeros(0, bool)


@pytest.mark.parametrize("cuts", [1, 3, 7])
@pytest.mark.parametrize("name", ["c3", "c4", "fuzz", "edge"])
def test_goldens_in_batches_equal_the_flow_table_of_the_concatenation(name, cuts):
    """With room for every flow and no expiry, (class, key, packets, bytes) in record order are the
    per-batch table's over the whole stream, and first / last map through the batches' starts. The
    golden and half of it again, so that flows recur in later batches."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    reps_n = n0 + n0 // 2
    k = ["c3", "c4", "fuzz", "edge"].index(name) + cuts
    for flags, selected in ((ALL_FLAGS[k % 4], False), (ALL_FLAGS[(k + 1) % 4], True), (ALL_FLAGS[(k + 2) % 4], True)):
        host, ref, bounds, bits = run_golden(name, reps_n, cuts, flags, selected)
        desc = np.resize(g["desc"], reps_n)
        sel = fr.pack_bits(bits) if selected else None
        _, flows, res = abi.flow_table_host(g["data"], desc, abi.FlowTableOpts(flags, 0, reps_n, 0), sel)
        recs = host.records()
        assert len(recs) == res["n_flows"] == host.header()["n_flows"] and res["overflow_packets"] == 0
        for field in ("klass", "key", "packets", "bytes"):
            assert (recs[field] == flows[field]).all(), field
        starts = bounds[:-1]
        assert (starts[recs["first_batch"]] + recs["first"] == flows["first"]).all()
        assert (starts[recs["last_batch"]] + recs["last"] == flows["last"]).all()
        assert host.header()["seq"] == cuts
        if cuts > 1 and not selected:
            assert (recs["last_batch"] > recs["first_batch"]).any()   # flows did recur


def test_overflow_at_the_exact_boundary():
    """flow_cap equal to the distinct flows: no overflow. One less: exactly the last new flow and
    its packets overflow, in whichever batch it first appears, and again when it comes back."""
    name, flags = "fuzz", ftr.BIDIRECTIONAL
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    reps_n = n0 + n0 // 2
    inputs, nbytes, klass = golden_keys(name)
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    nf = ftr.expected(inputs, nbytes, klass, lens, flags)["result"]["n_flows"]
    host, ref, _, _ = run_golden(name, reps_n, 3, flags, False, flow_cap=nf)
    h = host.header()
    assert h["n_flows"] == nf and h["overflow_packets"] == 0 and h["overflow_bytes"] == 0
    host, ref, _, _ = run_golden(name, reps_n, 3, flags, False, flow_cap=nf - 1)
    h = host.header()
    assert h["n_flows"] == nf - 1 and h["overflow_packets"] > 0 and h["seq"] == 3
    # the flow left out is the last of the whole stream's flows, and its packets are what overflowed
    whole = ftr.expected(np.resize(inputs, (reps_n, inputs.shape[1])), np.resize(nbytes, reps_n), np.resize(klass, reps_n),
                         np.resize(lens, reps_n), flags)
    last = whole["flows"][-1]
    assert h["overflow_packets"] == int(last["packets"].sum()) and h["overflow_bytes"] == int(last["bytes"].sum())
    assert (host.records()["key"] == whole["flows"]["key"][:-1]).all()


def _tcp(src, dst, sp, dp, pad=0):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(16 + pad)


def pack_frames(frames):
    """(data, desc): the frames back to back, each at an odd offset."""
    data, desc = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)
        desc.append(len(data) | len(f) << 48)
        data += f
    return np.frombuffer(bytes(data), np.uint8), np.array(desc, np.uint64)


class Pair:
    """The host tracker and the restatement side by side over crafted frames."""

    def __init__(self, flow_cap, flags=0, slots=0):
        self.host, self.ref = abi.HostFlowTracker(flow_cap, flags, slots), fkr.Tracker(flow_cap, flags, slots)
        self.flags = flags

    def update(self, frames, ts=None, batch_ts=0, select=None):
        data, desc = pack_frames(frames)
        inputs, nbytes, klass = fr.key_of_frames(frames, bool(self.flags & ftr.L3_ONLY)) if frames else \
            (np.zeros((0, 36), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64))
        t = None if ts is None else np.asarray(ts, np.uint64)
        fid, res = self.host.update(data, desc, select, t, batch_ts)
        want = self.ref.update(inputs, nbytes, klass, [len(f) for f in frames], select, t, batch_ts)
        assert res == want["result"], (res, want["result"])
        assert (fid == want["flow_id"]).all()
        same_state(self.host, self.ref)
        return fid, res

    def expire(self, now, idle, expired_cap=None):
        exp, remap, res = self.host.expire(now, idle, expired_cap)
        want = self.ref.expire(now, idle, expired_cap)
        assert res == want["result"], (res, want["result"])
        nb = res["n_flows_before"]
        assert (remap[:nb] == want["remap"]).all() and (remap[nb:] == 0xEEEEEEEE).all()   # nothing written past n_flows_before
        if expired_cap is not None:
            assert exp.tobytes() == want["expired"].tobytes()
        same_state(self.host, self.ref)
        return exp, remap, res


def flow(k):
    return _tcp([10, 0, k >> 8, k & 255], [10, 9, 0, 1], 1000 + k, 80)


def test_expire_boundaries_truncation_remap_and_reappearance():
    p = Pair(16)
    p.update([flow(0), flow(1), flow(2), flow(3), flow(1)], ts=[100, 200, 300, 400, 90])   # flow 1's last_ts is 90: its last packet's
    assert p.host.records()["last_ts"].tolist() == [100, 90, 300, 400]
    # now - last_ts == idle stays, + 1 goes; last_ts > now stays
    _, remap, res = p.expire(now=350, idle=250, expired_cap=8)   # 350 - 100 = 250: flow 0 stays; 350 - 90 = 260: flow 1 goes
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (1, 1, 3) and remap[:4].tolist() == [0, fkr.EXPIRED, 1, 2]
    exp, remap, res = p.expire(now=351, idle=250, expired_cap=8)   # 351 - 100 = 251: flow 0 goes; 400 > 351 stays
    assert res["n_expired"] == 1 and exp["last_ts"].tolist() == [100] and remap[:3].tolist() == [fkr.EXPIRED, 0, 1]
    _, _, res = p.expire(now=0, idle=0, expired_cap=8)   # every last_ts is above now
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (0, 0, 2)
    # a removed key that appears again is a new flow at the end; the flows that stayed are found
    fid, res = p.update([flow(3), flow(1), flow(2), flow(0)], batch_ts=500)
    assert fid.tolist() == [1, 2, 0, 3] and res["new_flows"] == 2
    assert p.host.records()["first_batch"].tolist() == [0, 0, 1, 1]
    # expired_cap truncates in ascending flow number; the rest stay and go with the next call
    p.update([flow(k) for k in range(4, 10)], batch_ts=10)
    exp, remap, res = p.expire(now=1000, idle=100, expired_cap=4)
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (10, 4, 6) and remap[:10].tolist() == [fkr.EXPIRED] * 4 + list(range(6))
    exp, remap, res = p.expire(now=1000, idle=100, expired_cap=0)   # room for none: nothing is lost
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (6, 0, 6)
    # expired == NULL: every idle flow is dropped
    p.update([flow(20)], batch_ts=1000)
    _, remap, res = p.expire(now=1000, idle=100, expired_cap=None)
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (6, 6, 1) and remap[:7].tolist() == [fkr.EXPIRED] * 6 + [0]
    fid, res = p.update([flow(20), flow(4)], batch_ts=1001)
    assert fid.tolist() == [0, 1] and res["new_flows"] == 1
    assert p.host.header()["seq"] == 5


def test_a_full_table_and_an_empty_batch():
    """flow_cap = slots = 128 fills every slot; a 129th flow overflows; the same 128 keys again are all found."""
    p = Pair(128, slots=128)
    fid, res = p.update([flow(k) for k in range(128)], batch_ts=1)
    assert fid.tolist() == list(range(128)) and res["n_flows"] == 128
    fid, res = p.update([flow(128), flow(5)], batch_ts=2)
    assert fid.tolist() == [abi.FLOW_ID_OVERFLOW, 5] and (res["overflow_flows"], res["overflow_packets"], res["overflow_bytes"]) == (1, 1, 54)
    fid, res = p.update([flow(k) for k in reversed(range(128))], batch_ts=3)
    assert fid.tolist() == list(reversed(range(128))) and res["new_flows"] == 0
    fid, res = p.update([], batch_ts=4)   # n == 0 is a batch: the sequence number advances
    assert res["seq"] == 3 and p.host.header()["seq"] == 4 and res["n_flows"] == 128
    # no key, unselected
    sel = np.array([0b101], np.uint64)
    fid, res = p.update([bytes(20), flow(1), flow(2)], batch_ts=5, select=sel)
    assert fid.tolist() == [abi.FLOW_ID_NONE, abi.FLOW_ID_UNSELECTED, 2] and p.host.header()["none_packets"] == 1


def test_layout_and_scratch_sizes():
    for cap, slots, want in ((1, 0, 128), (64, 0, 128), (65, 0, 256), (100, 128, 128), (128, 128, 128), (4096, 4096, 4096),
                             (4097, 0, 16384), (1 << 30, 0, 1 << 31)):
        lay = abi.flow_track_layout(cap, slots)
        assert lay["slots"] == want == fkr.Tracker(cap, 0, slots).slots
        assert lay["header"] == 0 and lay["records"] >= 128 and lay["slot_words"] - lay["records"] >= 104 * cap
        assert lay["total"] - lay["slot_words"] >= 4 * want
        assert all(lay[k] % 256 == 0 for k in ("records", "slot_words", "total"))
    L = abi.lib()
    s = abi.FlowTrackSizes()
    for cap, slots in ((0, 0), (0, 128), (0xFFFFFFFC, 1 << 31), (0xFFFFFFFF, 1 << 31), ((1 << 30) + 1, 0), (100, 64), (129, 128),
                       (100, 200), (1, 3 << 10)):
        assert L.bt_flow_track_layout(cap, slots, ctypes.byref(s)) == BT_E_INVALID_ARGUMENT, (cap, slots)
    assert L.bt_flow_track_layout(1, 0, None) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_track_layout(0xFFFFFFFB, 1 << 31, ctypes.byref(s)) == BT_E_INVALID_ARGUMENT   # slots is a u32 power of two
    assert L.bt_flow_track_layout(1 << 31, 1 << 31, ctypes.byref(s)) == 0 and s.total > 104 << 31   # the largest flow_cap
    # an update's scratch: the per-batch table's at auto slots, n flow records, its result, the map, the partials
    ns = [0, 1, 63, 64, 65, 255, 256, 257, 16384, 16385, 1 << 24, 1 << 30]
    sizes = [abi.flow_track_scratch_bytes(n) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(x % 256 == 0 for x in sizes)
    for n, size in zip(ns, sizes):
        assert size >= abi.flow_table_scratch_bytes(n, 0) + 80 * n + 72 + 4 * n + 40 * ((n + 255) // 256)
    b = ctypes.c_uint64(0)
    assert L.bt_flow_track_scratch_bytes((1 << 30) + 1, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_track_scratch_bytes(1, None) == BT_E_INVALID_ARGUMENT
    caps = [1, 255, 256, 257, 1 << 20, 1 << 31]
    sizes = [abi.flow_track_expire_scratch_bytes(c) for c in caps]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(x % 256 == 0 for x in sizes)
    assert all(size >= 104 * c + 24 * ((c + 255) // 256) for c, size in zip(caps, sizes))
    assert L.bt_flow_track_expire_scratch_bytes(0, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_track_expire_scratch_bytes((1 << 31) + 1, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowTrackRec.itemsize == 104 and fkr.FLOW_TRACK_REC == abi.FlowTrackRec
    assert abi.FlowTrackRec.fields["first_ts"][1] == 88 and abi.FlowTrackRec.fields["packets"][1] == 56
    assert re.search(r"typedef struct bt_flow_track_rec \{\s*/\* 104 B", src)
    sizes = {abi.FlowTrackHdr: 128, abi.FlowTrackOpts: 16, abi.FlowTrackSizes: 40, abi.FlowTrackUpdate: 16, abi.FlowTrackResult: 64,
             abi.FlowTrackOut: 16, abi.FlowTrackExpireResult: 32, abi.FlowTrackExpireOut: 32}
    for cls, size in sizes.items():
        assert ctypes.sizeof(cls) == size, cls
    assert (abi.FlowTrackHdr.selected_packets.offset, abi.FlowTrackHdr.selected_bytes.offset) == (24, 56)
    assert (abi.FlowTrackResult.seq.offset, abi.FlowTrackResult.keyed_bytes.offset) == (32, 40)
    assert abi.FLOW_ID_EXPIRED == fkr.EXPIRED == 0xFFFFFFFB < abi.FLOW_ID_OVERFLOW
    assert re.search(r"#define BT_FLOW_ID_EXPIRED\s+0xFFFFFFFBu", src)
    assert abi.FLOW_TRACK_MAGIC == fkr.MAGIC and re.search(r"#define BT_FLOW_TRACK_MAGIC\s+0x4B525446u", src)
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_track_layout", "bt_flow_track_scratch_bytes", "bt_flow_track_expire_scratch_bytes",
                 "bt_flow_track_init_device", "bt_flow_track_update_device", "bt_flow_track_expire_device",
                 "bt_flow_track_init_host", "bt_flow_track_update_host", "bt_flow_track_expire_host", "bt_flow_track_forget"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    for name in ("bt_time_flow_track", "bt_time_flow_track_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name)
    assert abi.lib().bt_abi_version() == 2


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason."""
    L = abi.lib()
    lay = abi.flow_track_layout(64)
    raw = (ctypes.c_uint8 * (lay["total"] + 512))()
    st = (ctypes.addressof(raw) + 255) & ~255
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    res = (ctypes.c_uint64 * 8)()
    rp = ctypes.addressof(res)
    need = abi.flow_track_scratch_bytes(2)
    sraw = (ctypes.c_uint8 * (need + 512))()
    sp = (ctypes.addressof(sraw) + 255) & ~255

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def init(word, state=st, nbytes=lay["total"], opts=abi.FlowTrackOpts(0, 64, 0, 0)):
        said(L.bt_flow_track_init_device(None, state, nbytes, ctypes.byref(opts) if opts is not None else None, None), word)

    init("null context")
    init("null state", state=None)
    init("state is not 256-byte aligned", state=st + 128)
    init("null opts", opts=None)
    init("unknown flag", opts=abi.FlowTrackOpts(4, 64, 0, 0))
    init("flow_cap == 0", opts=abi.FlowTrackOpts(0, 0, 0, 0))
    init("sentinels", opts=abi.FlowTrackOpts(0, 0xFFFFFFFC, 1 << 31, 0))
    init("power of two", opts=abi.FlowTrackOpts(0, 64, 129, 0))
    init("below 128", opts=abi.FlowTrackOpts(0, 64, 64, 0))
    init("slots below flow_cap", opts=abi.FlowTrackOpts(0, 300, 256, 0))
    init("below the layout", nbytes=lay["total"] - 1)
    init("below the layout", opts=abi.FlowTrackOpts(0, 65, 0, 0))

    def good():
        return (abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0),
                abi.FlowTrackUpdate(None, 0), abi.FlowTrackOut(None, rp))

    def update(word, frames, upd, out, state=st, scratch=sp, nbytes=need):
        said(L.bt_flow_track_update_device(None, state, ctypes.byref(frames) if frames is not None else None, None,
                                           ctypes.byref(upd) if upd is not None else None, scratch, nbytes,
                                           ctypes.byref(out) if out is not None else None, None), word)

    f, u, o = good()
    update("not an initialised tracker", f, u, o)   # nothing else is wrong: no device call has initialised this address
    update("null state", f, u, o, state=None)
    update("state is not 256-byte aligned", f, u, o, state=st + 8)
    update("null frames", None, u, o)
    update("null upd", f, None, o)
    update("null out", f, u, None)
    update("null result", f, u, abi.FlowTrackOut(None, None))
    update("result is not 8-byte aligned", f, u, abi.FlowTrackOut(None, rp + 4))
    update("flow_id is not 4-byte aligned", f, u, abi.FlowTrackOut(rp + 2, rp))
    update("ts is not 8-byte aligned", f, abi.FlowTrackUpdate(rp + 4, 0), o)
    update("scratch is not 256-byte aligned", f, u, o, scratch=sp + 64)
    update("null scratch", f, u, o, scratch=None)
    update("below the need", f, u, o, nbytes=need - 1)
    for flags in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f, u, o = good()
        f.flags = flags
        update("BT_BATCH_PREFIXES", f, u, o)
    f, u, o = good()
    f.n = (1 << 30) + 1
    update("n above 2^30", f, u, o)
    f, u, o = good()
    f.bytes = 0
    update("bytes == 0", f, u, o)
    f, u, o = good()
    f.desc_format = 2
    update("desc_format", f, u, o)
    f, u, o = good()
    f.base = None
    update("null packet buffer", f, u, o)

    xneed = abi.flow_track_expire_scratch_bytes(64)
    xres = (ctypes.c_uint64 * 4)()
    xp = ctypes.addressof(xres)

    def expire(word, out, state=st, scratch=sp, nbytes=xneed):
        said(L.bt_flow_track_expire_device(None, state, 10, 5, scratch, nbytes, ctypes.byref(out) if out is not None else None,
                                           None), word)

    ok = abi.FlowTrackExpireOut(None, 0, 0, None, xp)
    expire("not an initialised tracker", ok)
    expire("null state", ok, state=None)
    expire("state is not 256-byte aligned", ok, state=st + 16)
    expire("null out", None)
    expire("null result", abi.FlowTrackExpireOut(None, 0, 0, None, None))
    expire("result is not 8-byte aligned", abi.FlowTrackExpireOut(None, 0, 0, None, xp + 4))
    expire("expired is not 8-byte aligned", abi.FlowTrackExpireOut(xp + 4, 1, 0, None, xp))
    expire("remap is not 4-byte aligned", abi.FlowTrackExpireOut(None, 0, 0, xp + 2, xp))
    expire("null expired with expired_cap != 0", abi.FlowTrackExpireOut(None, 1, 0, None, xp))
    expire("null scratch", ok, scratch=None)
    expire("scratch is not 256-byte aligned", ok, scratch=sp + 32)
    assert bytes(raw) == bytes(len(raw)) and bytes(sraw) == bytes(len(sraw)) and bytes(res) == bytes(64)

    # the host forms: a state that is not an initialised tracker, by its header and by state_bytes
    r = abi.FlowTrackResult()
    upd = abi.FlowTrackUpdate(None, 0)

    def host_update(word, state=st, nbytes=lay["total"], u=upd, result=r):
        said(L.bt_flow_track_update_host(state, nbytes, ctypes.addressof(data), 256, ctypes.addressof(desc), 2, None,
                                         ctypes.byref(u) if u is not None else None, None,
                                         ctypes.byref(result) if result is not None else None), word)

    host_update("not an initialised tracker")   # zeros
    said(L.bt_flow_track_expire_host(st, lay["total"], 1, 1, ctypes.byref(ok)), "not an initialised tracker")
    said(L.bt_flow_track_init_host(st, lay["total"] - 1, ctypes.byref(abi.FlowTrackOpts(0, 64, 0, 0))), "below the layout")
    assert L.bt_flow_track_init_host(st, lay["total"], ctypes.byref(abi.FlowTrackOpts(0, 64, 0, 0))) == 0
    host_update("null state", state=None)
    host_update("state_bytes below the header's layout", nbytes=lay["total"] - 1)
    host_update("state_bytes below the header", nbytes=64)
    host_update("null upd", u=None)
    host_update("null result", result=None)
    said(L.bt_flow_track_expire_host(st, lay["total"], 1, 1, None), "null out")
    said(L.bt_flow_track_expire_host(st, lay["total"], 1, 1, ctypes.byref(abi.FlowTrackExpireOut(None, 0, 0, None, None))), "null result")
    said(L.bt_flow_track_expire_host(st, lay["total"], 1, 1, ctypes.byref(abi.FlowTrackExpireOut(None, 3, 0, None, xp))),
         "null expired with expired_cap != 0")
    hdr = abi.FlowTrackHdr.from_address(st)
    for field, bad in (("magic", 0), ("flags", 8), ("flow_cap", 0), ("slots", 96), ("n_flows", 65)):
        keep = getattr(hdr, field)
        setattr(hdr, field, bad)
        host_update("the header does not hold one")
        setattr(hdr, field, keep)
    assert L.bt_flow_track_update_host(st, lay["total"], ctypes.addressof(data), 256, ctypes.addressof(desc), 2, None,
                                       ctypes.byref(upd), None, ctypes.byref(r)) == 0


def test_flowtrack_host_check_builds_and_passes(tmp_path):
    """tools/flowtrack_host_check.cpp: the layout, the argument checks and the host tracker under
    AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowtrack_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowtrack_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
