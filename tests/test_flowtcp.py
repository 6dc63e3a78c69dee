"""CPU: the per-flow TCP side table on the host (bt_flow_tcp_update_host, bt_flow_tcp_state,
bt_flow_track_expire_tcp_host, include/beatrice_gpu.h) against the restatement in flowtcp_ref.py
(flags, ok and fragment bits from the goldens' reference-made bt_rec, keys through flow_ref and
flowtab_ref), the ctypes layout of the new structs, and the refusals of the device calls, which
need no GPU."""
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
import flowtcp_ref as tr
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)
GOLDENS = ["c3", "c4", "fuzz", "edge"]
U64_MAX = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def golden_tcp(name, flags):
    """Per packet of a golden: flow_ref's key triple under the flags' L3_ONLY, (contributes, flags byte), direction."""
    g, _ = load_golden(name)
    keys = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
    tcp, fl = tr.tcp_of_rec(g["rec"])
    return keys, tcp, fl, tr.directions(*keys, flags)


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowTcpRec.itemsize == 16 and tr.TCP_REC == abi.FlowTcpRec
    assert re.search(r"typedef struct bt_flow_tcp_rec \{\s*/\* 16 B", src)
    assert ctypes.sizeof(abi.FlowTcpResult) == 32 and re.search(r"typedef struct bt_flow_tcp_result \{\s*/\* 32 B", src)
    assert ctypes.sizeof(abi.FlowTrackExpireTcp) == 24 and re.search(r"typedef struct bt_flow_track_expire_tcp \{\s*/\* 24 B", src)
    assert abi.FlowTcpResult.bad_ids.offset == 20 and abi.FlowTrackExpireTcp.closed_idle.offset == 16
    for name, bit in (("FIN", 1), ("SYN", 2), ("RST", 4), ("PSH", 8), ("ACK", 16)):
        assert re.search(rf"#define BT_TCPF_{name}\s+0x{bit:02x}u", src) and getattr(abi, "TCPF_" + name) == getattr(tr, name) == bit
    enum = re.search(r"enum \{ (BT_TCP_NONE = 0.*?) \};", src, flags=re.S).group(1)
    got = {m[0]: int(m[1]) for m in re.findall(r"BT_TCP_([A-Z]+) = (\d)", enum)}
    assert got == {"NONE": 0, "OPENING": 1, "ESTABLISHED": 2, "CLOSING": 3, "CLOSED": 4, "RESET": 5, "MIDSTREAM": 6}
    assert all(getattr(abi, "TCP_" + k) == v == getattr(tr, k) for k, v in got.items())
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_tcp_update_device", "bt_flow_tcp_update_host", "bt_flow_tcp_state", "bt_flow_track_expire_tcp_scratch_bytes",
                 "bt_flow_track_expire_tcp_device", "bt_flow_track_expire_tcp_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    assert "bt_time_flow_tcp" in abi.EXPORTS and hasattr(abi.lib(), "bt_time_flow_tcp")
    assert abi.lib().bt_abi_version() == 2
    for cap in (1, 255, 256, 257, 1 << 20):
        assert abi.flow_track_expire_tcp_scratch_bytes(cap) >= abi.flow_track_expire_scratch_bytes(cap) + 16 * cap
        assert abi.flow_track_expire_tcp_scratch_bytes(cap) % 256 == 0
    b = ctypes.c_uint64(0)
    assert abi.lib().bt_flow_track_expire_tcp_scratch_bytes(0, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert abi.lib().bt_flow_track_expire_tcp_scratch_bytes(1, None) == BT_E_INVALID_ARGUMENT


def test_state_over_every_flag_pair_in_both_modes():
    L = abi.lib()
    for flags in ALL_FLAGS:
        for fwd in range(256):
            got = [L.bt_flow_tcp_state(fwd, rev, flags) for rev in range(256)]
            assert got == [tr.state(fwd, rev, flags) for rev in range(256)], (flags, fwd)
    # the handshake, the close and the reset, by name
    B = ftr.BIDIRECTIONAL
    assert abi.flow_tcp_state(0, 0, B) == abi.TCP_NONE
    assert abi.flow_tcp_state(tr.SYN, 0, B) == abi.TCP_OPENING
    assert abi.flow_tcp_state(tr.SYN | tr.ACK, tr.SYN | tr.ACK, B) == abi.TCP_ESTABLISHED
    assert abi.flow_tcp_state(tr.SYN | tr.ACK | tr.FIN, tr.SYN | tr.ACK, B) == abi.TCP_CLOSING
    assert abi.flow_tcp_state(tr.SYN | tr.ACK | tr.FIN, tr.SYN | tr.ACK | tr.FIN, B) == abi.TCP_CLOSED
    assert abi.flow_tcp_state(tr.SYN | tr.ACK | tr.FIN, tr.RST, B) == abi.TCP_RESET
    assert abi.flow_tcp_state(tr.ACK | tr.PSH, tr.ACK, B) == abi.TCP_MIDSTREAM
    assert abi.flow_tcp_state(tr.SYN, 0, 0) == abi.TCP_OPENING and abi.flow_tcp_state(tr.SYN | tr.ACK, 0, 0) == abi.TCP_ESTABLISHED
    assert abi.flow_tcp_state(tr.ACK | tr.FIN, 0, 0) == abi.TCP_CLOSED and abi.flow_tcp_state(0, tr.FIN, 0) == abi.TCP_CLOSING


@pytest.mark.parametrize("name", GOLDENS)
def test_the_python_walk_agrees_with_the_reference_records(name):
    """tcp_of_frame (used where no golden record exists) against tcp_of_rec on every golden frame."""
    g, _ = load_golden(name)
    off, ln = (g["desc"] & fr.MASK48).astype(np.int64), (g["desc"] >> np.uint64(48)).astype(np.int64)
    tcp, fl = tr.tcp_of_rec(g["rec"])
    wtcp, wfl = tr.tcp_of_frames([g["data"][o:o + m].tobytes() for o, m in zip(off, ln)])
    assert (tcp == wtcp).all() and (fl == wfl).all()
    counts = {"c3": 2082, "c4": 1068, "fuzz": 685, "edge": 69}
    assert int(((g["rec"][:, 25] & fr.L_TCP) != 0).sum()) == counts[name]
    if name == "fuzz":   # IPv4 fragments with a parsed TCP layer: the fragment rule is exercised
        assert int((((g["rec"][:, 25] & fr.L_TCP) != 0) & ~tcp).sum()) == 18
    if name == "c3":
        f = g["rec"][(g["rec"][:, 25] & fr.L_TCP) != 0, 81]
        assert (int((f & 2 != 0).sum()), int((f & 1 != 0).sum()), int((f & 4 != 0).sum())) == (1052, 1044, 984)
        assert len(np.unique(f)) == 256


def run_cuts(name, cuts, flags):
    """The golden and half of it again in `cuts` batches: the host tracker numbers the packets, the host
    update fills the side table; the restatement does the same from the reference records."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    reps_n = n0 + n0 // 2
    desc, reps = np.resize(g["desc"], reps_n), np.resize(np.arange(n0), reps_n)
    keys, tcp, fl, dirs = golden_tcp(name, flags)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    bounds = np.linspace(0, reps_n, cuts + 1).astype(int)
    host, ref = abi.HostFlowTracker(reps_n, flags), fkr.Tracker(reps_n, flags)
    want = np.zeros(reps_n, tr.TCP_REC)
    total = dict.fromkeys(("tcp_packets", "syn_packets", "fin_packets", "rst_packets"), 0)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        r = reps[lo:hi]
        fid, _ = host.update(g["data"], desc[lo:hi], batch_ts=1)
        wid = ref.update(keys[0][r], keys[1][r], keys[2][r], lens[lo:hi], batch_ts=1)["flow_id"]
        assert (fid == wid).all()
        res = host.tcp_update(g["data"], desc[lo:hi], fid)
        wres = tr.update(want, wid, tcp[r], fl[r], dirs[r])
        assert res == wres, (name, cuts, flags, res, wres)
        for k in total:
            total[k] += res[k]
    assert host.tcp_table().tobytes() == want.tobytes(), (name, cuts, flags)
    return want, total


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_in_cuts_equal_the_restatement_and_the_concatenation(name):
    g, _ = load_golden(name)
    for flags in ALL_FLAGS:
        whole, total = run_cuts(name, 1, flags)
        assert total["tcp_packets"] > 0 and whole["flags"].any()
        for cuts in (2, 7):
            got, tot = run_cuts(name, cuts, flags)
            assert got.tobytes() == whole.tobytes() and tot == total, (name, cuts, flags)
        if flags & ftr.BIDIRECTIONAL and name in ("c4", "fuzz"):   # c3 and edge have no TCP packet from the larger endpoint
            assert whole["flags"][:, 1].any()   # some packets did count in the reverse direction
        if not flags & ftr.BIDIRECTIONAL:
            assert not whole["flags"][:, 1].any()


def _tcp(src, dst, sp, dp, flags, vlan=0):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    l4 = sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, flags]) + bytes(6)
    tag = b"".join(b"\x81\x00\x00\x05" for _ in range(vlan))
    return bytes(12) + tag + b"\x08\x00" + ip + l4


A, B = [10, 0, 0, 1], [10, 0, 0, 2]


def up(k, flags):
    """A packet of conversation k from the smaller endpoint (direction 0 when bidirectional)."""
    return _tcp(A, B, 1000 + k, 80, flags)


def down(k, flags):
    return _tcp(B, A, 80, 1000 + k, flags)


def pack_frames(frames):
    """(data, desc): the frames back to back, each at an odd offset."""
    data, desc = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)
        desc.append(len(data) | len(f) << 48)
        data += f
    return np.frombuffer(bytes(data), np.uint8), np.array(desc, np.uint64)


def test_sentinels_and_ids_at_or_past_flow_cap():
    frames = [up(0, tr.SYN), down(0, tr.SYN | tr.ACK), up(1, tr.RST), up(2, tr.FIN), up(3, tr.SYN), up(4, tr.SYN), up(5, tr.SYN),
              bytes(60)]
    data, desc = pack_frames(frames)
    ids = np.array([1, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 3, 0xFFFFFFFC], np.uint32)
    table = np.zeros(3, abi.FlowTcpRec)   # id 3 is at flow_cap
    res = abi.flow_tcp_update_host(data, desc, ids, ftr.BIDIRECTIONAL, table)
    assert res == {"n": 8, "tcp_packets": 2, "syn_packets": 1, "fin_packets": 0, "rst_packets": 0, "bad_ids": 2, "reserved": [0, 0]}
    assert table["flags"].tolist() == [[0, 0], [tr.SYN, tr.SYN | tr.ACK], [0, 0]] and table["syn_packets"].tolist() == [0, 1, 0]
    want = np.zeros(3, tr.TCP_REC)
    tcp, fl = tr.tcp_of_frames(frames)
    assert tr.update(want, ids, tcp, fl, tr.directions(*fr.key_of_frames(frames), ftr.BIDIRECTIONAL)) == res
    assert want.tobytes() == table.tobytes()
    # flow_cap == 0 with a null table: every real id is a bad id; n == 0 writes the result
    res = abi.flow_tcp_update_host(data, desc, np.arange(8), 0, np.zeros(0, abi.FlowTcpRec))
    assert res["bad_ids"] == 8 and res["tcp_packets"] == 0
    assert abi.flow_tcp_update_host(data, desc[:0], ids[:0], 0, table)["n"] == 0
    # L3_ONLY changes the key (no ports), never who contributes; a fragment and a UDP packet do not
    frag = bytearray(up(7, tr.SYN))
    frag[20] = 0x20   # MF
    udp = bytearray(up(8, tr.SYN))
    udp[23] = 17
    data, desc = pack_frames([bytes(frag), bytes(udp), _tcp(A, B, 9, 9, tr.FIN | tr.ACK, vlan=2), _tcp(A, B, 9, 9, tr.PSH, vlan=3)])
    table = np.zeros(1, abi.FlowTcpRec)
    res = abi.flow_tcp_update_host(data, desc, np.zeros(4, np.uint32), ftr.L3_ONLY, table)
    assert (res["tcp_packets"], res["fin_packets"]) == (1, 1) and table["flags"].tolist() == [[tr.FIN | tr.ACK, 0]]
    # `bytes` cutting the TCP header: the layer is still parsed from the length, the missing flags byte reads as zero
    cut = int(desc[2] & fr.MASK48) + 14 + 8 + 20 + 13
    table[:] = 0
    res = abi.flow_tcp_update_host(data, desc[2:3], np.zeros(1, np.uint32), 0, table, nbytes=cut)
    assert res["tcp_packets"] == 1 and res["fin_packets"] == 0 and not table["flags"].any()
    res = abi.flow_tcp_update_host(data, desc[2:3], np.zeros(1, np.uint32), 0, table, nbytes=cut - 13 - 11)   # the protocol byte is gone
    assert res["tcp_packets"] == 0


class TcpPair:
    """The host tracker with its side table and the restatement side by side over crafted frames."""

    def __init__(self, flow_cap, flags=ftr.BIDIRECTIONAL):
        self.host, self.ref, self.flags = abi.HostFlowTracker(flow_cap, flags), fkr.Tracker(flow_cap, flags), flags
        self.want = np.zeros(flow_cap, tr.TCP_REC)

    def update(self, frames, ts):
        data, desc = pack_frames(frames)
        keys = fr.key_of_frames(frames, bool(self.flags & ftr.L3_ONLY))
        t = np.asarray(ts, np.uint64)
        fid, _ = self.host.update(data, desc, ts=t)
        wid = self.ref.update(*keys, [len(f) for f in frames], None, t)["flow_id"]
        assert (fid == wid).all()
        tcp, fl = tr.tcp_of_frames(frames)
        res = self.host.tcp_update(data, desc, fid)
        assert res == tr.update(self.want, wid, tcp, fl, tr.directions(*keys, self.flags))
        self.same()
        return fid

    def same(self):
        assert self.host.header() == self.ref.header()
        lay = self.host.layout
        recs = self.host.state[lay["records"]:lay["records"] + 104 * self.host.flow_cap]
        assert recs.tobytes() == self.ref.records(whole=True).tobytes()
        assert self.host.tcp_table().tobytes() == self.want.tobytes()

    def expire(self, now, idle, closed_idle, expired_cap=None):
        exp, exp_tcp, remap, res = self.host.expire_tcp(now, idle, closed_idle, expired_cap)
        want = tr.expire(self.ref, self.want, now, idle, closed_idle, expired_cap)
        assert res == want["result"], (res, want["result"])
        nb = res["n_flows_before"]
        assert (remap[:nb] == want["remap"]).all() and (remap[nb:] == 0xEEEEEEEE).all()
        if expired_cap is not None:
            assert exp.tobytes() == want["expired"].tobytes() and exp_tcp.tobytes() == want["expired_tcp"].tobytes()
        self.same()
        return exp, exp_tcp, remap, res

    def states(self):
        t = self.host.tcp_table()[:self.host.header()["n_flows"]]
        return [abi.flow_tcp_state(int(a), int(b), self.flags) for a, b in t["flags"]]


def test_expire_at_closed_idle_equals_the_plain_expire_when_it_never_applies():
    """closed_idle = 2^64 - 1: byte-equal to bt_flow_track_expire_host on state, remap, expired and result."""
    for name, flags, cap in (("c3", ftr.BIDIRECTIONAL, None), ("fuzz", 0, 7), ("c4", ftr.L3_ONLY | ftr.BIDIRECTIONAL, 0)):
        g, _ = load_golden(name)
        n = len(g["desc"])
        rng = np.random.default_rng(n)
        ts = rng.integers(0, 1000, n).astype(np.uint64)
        a, b = abi.HostFlowTracker(n, flags), abi.HostFlowTracker(n, flags)
        fid, _ = a.update(g["data"], g["desc"], ts=ts)
        b.update(g["data"], g["desc"], ts=ts)
        b.tcp_update(g["data"], g["desc"], fid)
        assert (b.tcp_table()["fin_packets"] > 0).any()   # there are closed connections that must stay
        before = b.tcp_table().copy()
        exp_a, remap_a, res_a = a.expire(1000, 500, cap)
        exp_b, exp_tcp, remap_b, res_b = b.expire_tcp(1000, 500, U64_MAX, cap)
        assert res_a == res_b and (remap_a == remap_b).all() and a.state.tobytes() == b.state.tobytes()
        assert res_a["n_expired"] > 0 or cap == 0
        nb = res_a["n_flows_before"]
        live = remap_a[:nb] != fkr.EXPIRED
        if cap is not None:
            assert exp_a.tobytes() == exp_b.tobytes()
            assert exp_tcp.tobytes() == before[:nb][~live][:len(exp_tcp)].tobytes()
        want = np.zeros(n, tr.TCP_REC)
        want[:int(live.sum())] = before[:nb][live]
        if res_a["n_expired"] == 0:
            want = before
        assert b.tcp_table().tobytes() == want.tobytes()


def test_closed_and_reset_connections_leave_at_closed_idle():
    p = TcpPair(8)
    # conversation 0: the whole life; 1: reset; 2: only one side has sent FIN; 3: established, open
    fid = p.update([up(0, tr.SYN), down(0, tr.SYN | tr.ACK), up(0, tr.ACK), up(0, tr.FIN | tr.ACK), down(0, tr.FIN | tr.ACK),
                    up(1, tr.SYN), up(1, tr.SYN), down(1, tr.RST | tr.ACK),
                    up(2, tr.SYN), down(2, tr.SYN | tr.ACK), down(2, tr.FIN | tr.ACK),
                    down(3, tr.SYN | tr.ACK), up(3, tr.SYN)], ts=[100] * 13)
    assert fid.tolist() == [0] * 5 + [1] * 3 + [2] * 3 + [3] * 2
    assert p.states() == [abi.TCP_CLOSED, abi.TCP_RESET, abi.TCP_CLOSING, abi.TCP_ESTABLISHED]
    t = p.host.tcp_table()
    assert t["syn_packets"][:4].tolist() == [1, 2, 1, 1] and t["fin_packets"][:4].tolist() == [2, 0, 1, 0]
    assert t["rst_packets"][:4].tolist() == [0, 1, 0, 0] and t["flags"][3].tolist() == [tr.SYN, tr.SYN | tr.ACK]
    # now - last_ts == closed_idle: nobody leaves; + 1: the closed and the reset one, not the half-closed one
    _, _, _, res = p.expire(now=110, idle=1000, closed_idle=10, expired_cap=8)
    assert (res["n_idle"], res["n_expired"]) == (0, 0)
    # expired_cap truncates without losing a flow: one now, the other with the next call
    exp, exp_tcp, remap, res = p.expire(now=111, idle=1000, closed_idle=10, expired_cap=1)
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (2, 1, 3) and remap[:4].tolist() == [fkr.EXPIRED, 0, 1, 2]
    assert exp_tcp["flags"].tolist() == [[tr.SYN | tr.ACK | tr.FIN, tr.SYN | tr.ACK | tr.FIN]] and exp_tcp["fin_packets"].tolist() == [2]
    assert p.states() == [abi.TCP_RESET, abi.TCP_CLOSING, abi.TCP_ESTABLISHED]
    exp, exp_tcp, remap, res = p.expire(now=111, idle=1000, closed_idle=10, expired_cap=1)
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (1, 1, 2) and exp_tcp["rst_packets"].tolist() == [1]
    assert p.host.tcp_table()["flags"][2:].sum() == 0   # zeros behind the live records
    # the closed conversation appears again: a new flow at the end with a zero side record, then its own flags
    fid = p.update([up(2, tr.ACK), up(0, tr.SYN)], ts=[120, 120])
    assert fid.tolist() == [0, 2] and p.states() == [abi.TCP_CLOSING, abi.TCP_ESTABLISHED, abi.TCP_OPENING]
    # the other side's FIN closes conversation 2; the idle rule still works beside it; expired == NULL drops
    p.update([up(2, tr.FIN | tr.ACK)], ts=[130])
    _, _, remap, res = p.expire(now=1121, idle=1000, closed_idle=10)
    assert (res["n_idle"], res["n_expired"], res["n_flows"]) == (3, 3, 0) and not p.host.tcp_table()["flags"].any()


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason."""
    L = abi.lib()
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    tcp = (ctypes.c_uint32 * 16)()
    res = (ctypes.c_uint64 * 4)()
    ip, tp, rp = ctypes.addressof(ids), ctypes.addressof(tcp), ctypes.addressof(res)

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def update(word, frames, flow_id=ip, flags=0, table=tp, cap=4, result=rp):
        said(L.bt_flow_tcp_update_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, flags, table, cap,
                                         result, None), word)

    update("null context", good())
    update("null frames", None)
    update("null flow_id", good(), flow_id=None)
    update("null tcp", good(), table=None)
    update("null result", good(), result=None)
    update("tcp is not 4-byte aligned", good(), table=tp + 2)
    update("flow_id is not 4-byte aligned", good(), flow_id=ip + 1)
    update("result is not 8-byte aligned", good(), result=rp + 4)
    update("unknown flag", good(), flags=4)
    for flags in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f = good()
        f.flags = flags
        update("BT_BATCH_PREFIXES", f)
    f = good()
    f.bytes = 0
    update("bytes == 0", f)
    f = good()
    f.desc_format = 2
    update("desc_format", f)
    f = good()
    f.base = None
    update("null packet buffer", f)
    f = good()
    f.n = 0
    update("null context", f, flow_id=None, table=None, cap=0)   # an empty batch needs no flow_id, flow_cap 0 no table

    def host(word, base=ctypes.addressof(data), d=ctypes.addressof(desc), flow_id=ip, flags=0, table=tp, cap=4, result=rp):
        said(L.bt_flow_tcp_update_host(base, 256, d, 2, flow_id, flags, table, cap, result), word)

    host("null base", base=None)
    host("null base", d=None)
    host("null flow_id", flow_id=None)
    host("null tcp", table=None)
    host("null result", result=None)
    host("tcp is not 4-byte aligned", table=tp + 1)
    host("result is not 8-byte aligned", result=rp + 4)
    host("unknown flag", flags=8)
    assert bytes(tcp) == bytes(64) and bytes(res) == bytes(32)

    lay = abi.flow_track_layout(64)
    raw = (ctypes.c_uint8 * (lay["total"] + 512))()
    st = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_track_expire_tcp_scratch_bytes(64)
    sraw = (ctypes.c_uint8 * (need + 512))()
    sp = (ctypes.addressof(sraw) + 255) & ~255
    side = (ctypes.c_uint32 * (4 * 64))()
    xp = ctypes.addressof(side)

    def expire(word, x, out, state=st, scratch=sp, nbytes=need):
        said(L.bt_flow_track_expire_tcp_device(None, state, 10, 5, ctypes.byref(x) if x is not None else None, scratch, nbytes,
                                               ctypes.byref(out) if out is not None else None, None), word)

    ok_x, ok_out = abi.FlowTrackExpireTcp(xp, None, 3), abi.FlowTrackExpireOut(None, 0, 0, None, rp)
    expire("not an initialised tracker", ok_x, ok_out)   # nothing else is wrong
    expire("null x", None, ok_out)
    expire("null tcp", abi.FlowTrackExpireTcp(None, None, 3), ok_out)
    expire("tcp is not 4-byte aligned", abi.FlowTrackExpireTcp(xp + 2, None, 3), ok_out)
    expire("expired_tcp is not 4-byte aligned", abi.FlowTrackExpireTcp(xp, xp + 1, 3), abi.FlowTrackExpireOut(rp, 1, 0, None, rp))
    expire("expired_tcp without expired", abi.FlowTrackExpireTcp(xp, xp, 3), ok_out)
    expire("null out", ok_x, None)
    expire("null state", ok_x, ok_out, state=None)
    expire("null result", ok_x, abi.FlowTrackExpireOut(None, 0, 0, None, None))
    expire("remap is not 4-byte aligned", ok_x, abi.FlowTrackExpireOut(None, 0, 0, rp + 2, rp))
    expire("null expired with expired_cap != 0", ok_x, abi.FlowTrackExpireOut(None, 1, 0, None, rp))
    expire("null scratch", ok_x, ok_out, scratch=None)
    expire("scratch is not 256-byte aligned", ok_x, ok_out, scratch=sp + 32)

    def xhost(word, x, out, state=st, nbytes=lay["total"]):
        said(L.bt_flow_track_expire_tcp_host(state, nbytes, 10, 5, ctypes.byref(x) if x is not None else None,
                                             ctypes.byref(out) if out is not None else None), word)

    xhost("not an initialised tracker", ok_x, ok_out)   # zeros
    assert L.bt_flow_track_init_host(st, lay["total"], ctypes.byref(abi.FlowTrackOpts(0, 64, 0, 0))) == 0
    xhost("null x", None, ok_out)
    xhost("null tcp", abi.FlowTrackExpireTcp(None, None, 3), ok_out)
    xhost("expired_tcp without expired", abi.FlowTrackExpireTcp(xp, xp, 3), ok_out)
    xhost("null out", ok_x, None)
    xhost("null result", ok_x, abi.FlowTrackExpireOut(None, 0, 0, None, None))
    xhost("null expired with expired_cap != 0", ok_x, abi.FlowTrackExpireOut(None, 2, 0, None, rp))
    xhost("null state", ok_x, ok_out, state=None)
    xhost("state_bytes below the header's layout", ok_x, ok_out, nbytes=lay["total"] - 1)
    assert L.bt_flow_track_expire_tcp_host(st, lay["total"], 10, 5, ctypes.byref(ok_x), ctypes.byref(ok_out)) == 0
    assert bytes(sraw) == bytes(len(sraw)) and bytes(side) == bytes(len(bytes(side)))


def test_flowtcp_host_check_builds_and_passes(tmp_path):
    """tools/flowtcp_host_check.cpp: the argument checks, the host update and the host expire under
    AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowtcp_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowtcp_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
