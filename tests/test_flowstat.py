"""CPU: the per-flow statistics side table on the host (bt_flow_stat_update_host, bt_flow_stat_rtt,
bt_flow_track_side_move_host, include/beatrice_gpu.h) against the restatement in flowstat_ref.py
(a Python layer walk for what a frame contributes, keys through flow_ref and flowtab_ref), the
ctypes layout of the new structs, and the refusals of the device calls, which need no GPU."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
import flowstat_ref as sr
import flowtab_ref as ftr
import flowtcp_ref as tr
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden
from flowstat_cases import arithmetic_frames, pack_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)
GOLDENS = ["c3", "c4", "fuzz", "edge"]
U64_MAX = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def golden_facts(name):
    """What every frame of a golden contributes, by the Python walk."""
    g, _ = load_golden(name)
    off, ln = (g["desc"] & fr.MASK48).astype(np.int64), (g["desc"] >> np.uint64(48)).astype(np.int64)
    return sr.facts_of_frames([g["data"][o:o + m].tobytes() for o, m in zip(off, ln)])


@functools.lru_cache(maxsize=None)
def golden_dirs(name, flags):
    """flow_ref's key triple of a golden under the flags' L3_ONLY, and every packet's direction."""
    g, _ = load_golden(name)
    keys = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
    return keys, tr.directions(*keys, flags)


def stamps(n, seed):
    """Per-packet timestamps that are not in order."""
    return (np.uint64(1000) + np.random.default_rng(seed).integers(0, 5000, n).astype(np.uint64))


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowStatRec.itemsize == 128 and sr.STAT_REC == abi.FlowStatRec
    assert re.search(r"typedef struct bt_flow_stat_rec \{\s*/\* 128 B", src)
    assert ctypes.sizeof(abi.FlowStatResult) == 32 and re.search(r"typedef struct bt_flow_stat_result \{\s*/\* 32 B", src)
    assert ctypes.sizeof(abi.FlowStatRttOut) == 32 and re.search(r"typedef struct bt_flow_stat_rtt_out \{\s*/\* 32 B", src)
    assert ctypes.sizeof(abi.FlowSideMove) == 48 and abi.FlowSideMove.rec_bytes.offset == 32
    assert abi.FlowStatResult.bad_ids.offset == 16 and abi.FlowStatRttOut.rtt_server.offset == 16
    enum = re.search(r"enum \{ (BT_FSEEN_TCP = 0x01.*?) \};", src, flags=re.S).group(1)
    got = {m[0]: int(m[1], 16) for m in re.findall(r"BT_FSEEN_([A-Z0-9_]+) = (0x[0-9a-f]+)", enum)}
    assert got == {"TCP": 1, "UDP": 2, "ICMP": 4, "ICMP6": 8, "OTHER": 0x10, "FRAGMENT": 0x20, "IP_OPTIONS": 0x40, "VLAN": 0x80, "L4": 0x100}
    assert all(getattr(abi, "FSEEN_" + k) == v == getattr(sr, "SEEN_" + k) for k, v in got.items())
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_stat_update_device", "bt_flow_stat_update_host", "bt_flow_stat_rtt", "bt_flow_track_side_move_scratch_bytes",
                 "bt_flow_track_side_move_device", "bt_flow_track_side_move_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    assert "bt_time_flow_stat" in abi.EXPORTS and hasattr(abi.lib(), "bt_time_flow_stat")
    assert abi.lib().bt_abi_version() == 2
    for cap in (1, 255, 256, 257, 1 << 20):
        for rb in (4, 16, 128, 256):
            need = abi.flow_track_side_move_scratch_bytes(cap, rb)
            assert need >= cap * rb + 24 * ((cap + 255) // 256) and need % 256 == 0
    assert abi.Context.flow_track_side_move_scratch_bytes(0, 4) == 0
    b = ctypes.c_uint64(0)
    for rb in (0, 2, 6, 260):
        assert abi.lib().bt_flow_track_side_move_scratch_bytes(1, rb, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert abi.lib().bt_flow_track_side_move_scratch_bytes(1, 4, None) == BT_E_INVALID_ARGUMENT


def run_cuts(name, cuts, flags, expire=None):
    """The golden and half of it again in `cuts` batches, batch b stamped per packet (even b) or as a
    whole (odd b): the host tracker numbers the packets, the host update fills the side table; the
    restatement does the same from the Python walk. expire = (now, idle, expired_cap): one expire
    behind the last batch, the side table moved by the host side move."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    reps_n = n0 + n0 // 2
    desc, reps = np.resize(g["desc"], reps_n), np.resize(np.arange(n0), reps_n)
    facts = golden_facts(name)
    keys, dirs = golden_dirs(name, flags)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    bounds = np.linspace(0, reps_n, cuts + 1).astype(int)
    host, ref = abi.HostFlowTracker(reps_n, flags), fkr.Tracker(reps_n, flags)
    got, want = np.zeros(reps_n, abi.FlowStatRec), np.zeros(reps_n, sr.STAT_REC)
    total = dict.fromkeys(("ip_packets", "l4_packets", "tcp_packets", "bad_ids"), 0)
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        r = reps[lo:hi]
        ts = stamps(hi - lo, lo) if b % 2 == 0 else None
        bts = 100 * (b + 1)
        fid, _ = host.update(g["data"], desc[lo:hi], ts=ts, batch_ts=bts)
        wid = ref.update(keys[0][r], keys[1][r], keys[2][r], lens[lo:hi], None, ts, bts)["flow_id"]
        assert (fid == wid).all()
        res = abi.flow_stat_update_host(g["data"], desc[lo:hi], fid, flags, got, ts=ts, batch_ts=bts)
        wres = sr.update(want, wid, facts[r], dirs[r], bts if ts is None else ts)
        assert res == wres, (name, cuts, flags, res, wres)
        for k in total:
            total[k] += res[k]
    assert got.tobytes() == want.tobytes(), (name, cuts, flags)
    if expire:
        now, idle, cap = expire
        _, remap, res = host.expire(now, idle, cap)
        assert res["n_expired"] > 0 and res["n_flows"] > 0 and (cap is None or res["n_idle"] > cap)
        gone = abi.flow_track_side_move_host(got, remap, res, res["n_expired"] + 3)
        wgone = sr.side_move(want, remap, res)
        assert gone.tobytes() == wgone.tobytes() and len(gone) == res["n_expired"]
        assert got.tobytes() == want.tobytes() and not got[res["n_flows"]:].tobytes().strip(b"\0")
    return want, total


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_in_cuts_equal_the_restatement_and_the_concatenation(name):
    for flags in ALL_FLAGS:
        whole, total = run_cuts(name, 1, flags)
        assert total["ip_packets"] > 0 and total["l4_packets"] >= total["tcp_packets"] > 0 and whole["len_sq"].any()
        if not flags & ftr.BIDIRECTIONAL:
            assert not (whole["seen"] >> 16).any() and not whole["len_max"][:, 1].any() and not whole["ack_ts_c"][:, 1].any()
        elif name in ("c4", "fuzz"):
            assert (whole["seen"] >> 16).any() and whole["payload_bytes"][:, 1].any()
    # per-packet and per-batch stamps alternate with the cuts, so only the order-free fields compare across cuts
    a, ta = run_cuts(name, 3, ftr.BIDIRECTIONAL)
    b, tb = run_cuts(name, 6, ftr.BIDIRECTIONAL)
    assert ta == tb
    for f in ("seen", "proto_max", "payload_packets", "ttl_max", "ttl_min_c", "len_max", "len_min_c", "payload_bytes", "len_sq"):
        assert (a[f] == b[f]).all(), f


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("name", GOLDENS)
def test_the_host_side_move_after_an_expire(name, flags):
    """Three batches, the first and the last stamped per packet 1000 .. 5999, the second 200; now = 5000,
    idle = 4650: the flows last seen before 350, in the second batch, leave. Once with room for all,
    once with expired_cap below the idle flows."""
    run_cuts(name, 3, flags, expire=(5000, 4650, None))
    run_cuts(name, 3, flags, expire=(5000, 4650, 2))


def test_the_side_move_is_generic_and_leaves_the_rest_alone():
    """Records of 4 and 20 bytes; entries at or past n_flows_before stay; bad remap values write nothing."""
    for dt in (np.dtype("<u4"), np.dtype([("a", "<u4", 5)])):
        side = np.arange(8 * (dt.itemsize // 4), dtype=np.uint32).view(dt).copy() if dt.itemsize > 4 else np.arange(1, 9, dtype=np.uint32)
        before = side.copy()
        remap = np.array([0, fkr.EXPIRED, 1, fkr.EXPIRED, 2, 7, 0xEEEEEEEE, 0xEEEEEEEE], np.uint32)
        res = {"n_flows_before": 6, "n_flows": 4, "n_idle": 2, "n_expired": 2, "status": 0}
        want = before.copy()
        wgone = sr.side_move(want, remap, res, 1)
        gone = abi.flow_track_side_move_host(side, remap, res, 1)
        assert gone.tobytes() == wgone.tobytes() == before[1:2].tobytes()
        assert side.tobytes() == want.tobytes()
        assert side[:3].tobytes() == before[[0, 2, 4]].tobytes() and not side[3:6].tobytes().strip(b"\0")   # 7 >= n_flows: dropped
        assert side[6:].tobytes() == before[6:].tobytes()
        # nothing expired, or a refused tracker (status 1, every count 0): nothing moves
        for res in ({"n_flows_before": 6, "n_flows": 6, "n_idle": 0, "n_expired": 0, "status": 0},
                    {"n_flows_before": 0, "n_flows": 0, "n_idle": 0, "n_expired": 0, "status": 1}):
            side = before.copy()
            assert len(abi.flow_track_side_move_host(side, remap, res, 4)) == 0 and side.tobytes() == before.tobytes()


def rec(**kw):
    r = np.zeros(1, abi.FlowStatRec)
    for k, v in kw.items():
        r[k + "_ts_c"][0] = [0 if t is None else U64_MAX - t for t in v]
    return r


def test_rtt_on_hand_made_records():
    none = {"has_initiator": 0, "initiator": 0, "server_valid": 0, "client_valid": 0, "rtt_server": 0, "rtt_client": 0}
    cases = [
        (rec(synack=[None, 7], ack=[9, None]), none),                                          # no SYN
        (rec(syn=[5, None]), dict(none, has_initiator=1)),                                     # SYN only
        (rec(syn=[None, 5]), dict(none, has_initiator=1, initiator=1)),
        (rec(syn=[5, None], synack=[None, 12], ack=[20, None]),
         dict(has_initiator=1, initiator=0, server_valid=1, client_valid=1, rtt_server=7, rtt_client=8)),
        (rec(syn=[None, 5], synack=[12, None], ack=[None, 20]),
         dict(has_initiator=1, initiator=1, server_valid=1, client_valid=1, rtt_server=7, rtt_client=8)),
        (rec(syn=[9, 9], synack=[11, 10], ack=[30, 40]),                                       # a tie goes to 0
         dict(has_initiator=1, initiator=0, server_valid=1, client_valid=1, rtt_server=1, rtt_client=20)),
        (rec(syn=[9, 8], synack=[11, 10], ack=[30, 40]),                                       # the earlier SYN wins
         dict(has_initiator=1, initiator=1, server_valid=1, client_valid=1, rtt_server=3, rtt_client=29)),
        (rec(syn=[10, None], synack=[None, 9], ack=[20, None]), dict(none, has_initiator=1)),  # SYN-ACK before the SYN
        (rec(syn=[10, None], synack=[None, 15], ack=[14, None]),                               # ACK before the SYN-ACK
         dict(none, has_initiator=1, server_valid=1, rtt_server=5)),
        (rec(syn=[10, None], synack=[None, 10], ack=[10, None]),                               # all at once: zero is valid
         dict(none, has_initiator=1, server_valid=1, client_valid=1)),
        (rec(syn=[0, None], synack=[None, U64_MAX - 1], ack=[U64_MAX - 1, None]),              # 0 and 2^64 - 2 are stamps
         dict(has_initiator=1, initiator=0, server_valid=1, client_valid=1, rtt_server=U64_MAX - 1, rtt_client=0)),
        (rec(syn=[5, None], synack=[12, None], ack=[None, 20]), dict(none, has_initiator=1)),  # the stamps of the wrong direction
    ]
    for r, want in cases:
        assert abi.flow_stat_rtt(r) == want == sr.rtt(r[0]), (r, want)
    d = abi.decode_flow_stat(cases[10][0])
    assert d["syn_ts"] == [0, None] and d["synack_ts"] == [None, U64_MAX - 1] and d["ttl_min"] == [None, None] and d["protocols"] == []
    assert abi.lib().bt_flow_stat_rtt(None, None) == BT_E_INVALID_ARGUMENT


def test_the_arithmetic_by_hand_and_by_the_restatement():
    frames = [f for f, _ in arithmetic_frames()]
    facts = sr.facts_of_frames(frames)
    # by hand: the restatement itself is held to the issue's numbers
    assert facts["payload"].tolist() == [100, 20, 12, 0, 0, 0, 0, 8, 8, 8, 0, 0, 0, 1, 0, 0, 65535 - 20 - 8, 0, 0]
    assert facts["ip"].tolist() == [True] * 17 + [False] * 2 and facts["l4"].tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 0]
    S = sr
    assert facts["seen"][:9].tolist() == [S.SEEN_TCP | S.SEEN_L4, S.SEEN_TCP | S.SEEN_L4, S.SEEN_UDP | S.SEEN_L4 | S.SEEN_VLAN, S.SEEN_ICMP,
                                          S.SEEN_ICMP6, S.SEEN_OTHER, S.SEEN_TCP | S.SEEN_FRAGMENT, S.SEEN_TCP | S.SEEN_L4,
                                          S.SEEN_TCP | S.SEEN_L4 | S.SEEN_IP_OPTIONS]
    assert facts["stamp"].tolist() == [2, 0, 3, 3, 3, 3, 3, 2, 2, 2, 2, 1, 2, 2, 3, 3, 3, 3, 3]
    assert facts["ttl"][:5].tolist() == [64, 33, 1, 255, 255]
    data, desc = pack_frames(frames)
    n = len(frames)
    ts = stamps(n, 1)
    for flags in ALL_FLAGS:
        dirs = tr.directions(*fr.key_of_frames(frames, bool(flags & ftr.L3_ONLY)), flags)
        for ids in (np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) % 3):
            got, want = np.zeros(n, abi.FlowStatRec), np.zeros(n, sr.STAT_REC)
            res = abi.flow_stat_update_host(data, desc, ids, flags, got, ts=ts)
            assert res == sr.update(want, ids, facts, dirs, ts) and got.tobytes() == want.tobytes(), flags
            assert res["ip_packets"] == 17 and res["l4_packets"] == 12 and res["tcp_packets"] == 10
    # one flow, bidirectional: the record in plain values
    got = np.zeros(1, abi.FlowStatRec)
    abi.flow_stat_update_host(data, desc, np.zeros(n, np.uint32), ftr.BIDIRECTIONAL, got, batch_ts=77)
    d = abi.decode_flow_stat(got[0])
    assert d["protocols"] == ["tcp", "udp", "icmp", "icmp6", "other"] and d["proto_max"] == 58
    assert d["ttl_min"] == [33, 1] and d["ttl_max"] == [255, 64] and d["syn_ts"] == [77, None] and d["synack_ts"] == [None, 77]
    # direction 1: the UDP packet and the SYN-ACK from B, and the IHL 4 packet, whose "destination" is its TCP ports (3.232.0.80 < A)
    rev = [len(frames[k]) for k in (2, 9, 11)]
    assert d["len_min"][1] == min(rev) and d["len_max"][0] == 14 + 20 + 20 + 100
    assert d["payload_packets"] == [6, 2] and d["payload_bytes"] == [100 + 20 + 8 + 8 + 1 + 65507, 12 + 8]
    assert d["len_sq"][1] == sum(x * x for x in rev)


def test_sentinels_bad_ids_a_starting_table_and_bytes():
    frames = [f for f, _ in arithmetic_frames()][:8]
    data, desc = pack_frames(frames)
    facts = sr.facts_of_frames(frames)
    ids = np.array([1, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 3, 0xFFFFFFFC], np.uint32)
    dirs = tr.directions(*fr.key_of_frames(frames), ftr.BIDIRECTIONAL)
    got, want = np.zeros(3, abi.FlowStatRec), np.zeros(3, sr.STAT_REC)   # id 3 is at flow_cap
    res = abi.flow_stat_update_host(data, desc, ids, ftr.BIDIRECTIONAL, got, batch_ts=5)
    assert res == sr.update(want, ids, facts, dirs, 5) and got.tobytes() == want.tobytes()
    assert res == {"n": 8, "ip_packets": 2, "l4_packets": 2, "tcp_packets": 2, "bad_ids": 2, "reserved": [0, 0, 0]}
    assert not got[0].tobytes().strip(b"\0") and not got[2].tobytes().strip(b"\0")
    # a non-zero starting table: the update adds to it and never resets it; the sums wrap
    start = np.zeros(3, sr.STAT_REC)
    start["seen"], start["ttl_max"], start["len_min_c"], start["syn_ts_c"] = 0x00100000, [[200, 0]] * 3, [[~np.uint32(20), 0]] * 3, U64_MAX
    start["payload_packets"], start["payload_bytes"], start["len_sq"] = 0xFFFFFFFF, U64_MAX - 3, U64_MAX
    got, want = start.copy().view(abi.FlowStatRec), start.copy()
    res = abi.flow_stat_update_host(data, desc, ids, ftr.BIDIRECTIONAL, got, ts=stamps(8, 3))
    assert res == sr.update(want, ids, facts, dirs, stamps(8, 3)) and got.tobytes() == want.tobytes()
    assert got["ttl_max"][1, 0] == 200 and got["syn_ts_c"][1, 0] == U64_MAX and got["payload_packets"][1, 0] == 1 and got["payload_bytes"][1, 0] < 200
    # flow_cap == 0 with a null table: every real id is a bad id; n == 0 writes the result
    res = abi.flow_stat_update_host(data, desc, np.arange(8), 0, np.zeros(0, abi.FlowStatRec))
    assert res["bad_ids"] == 8 and res["ip_packets"] == 0
    assert abi.flow_stat_update_host(data, desc[:0], ids[:0], 0, got)["n"] == 0
    # `bytes` cutting the first frame at every offset of its IP and TCP headers: the missing bytes read as zero
    off = int(desc[0] & fr.MASK48)
    for cut in range(14, 14 + 40 + 1):
        seen = bytes(frames[0][:cut]) + bytes(len(frames[0]) - cut)
        f1 = sr.facts_of_frames([seen])
        d1 = tr.directions(*fr.key_of_frames([seen]), ftr.BIDIRECTIONAL)
        got, want = np.zeros(1, abi.FlowStatRec), np.zeros(1, sr.STAT_REC)
        res = abi.flow_stat_update_host(data, desc[:1], [0], ftr.BIDIRECTIONAL, got, batch_ts=9, nbytes=off + cut)
        assert res == sr.update(want, [0], f1, d1, 9) and got.tobytes() == want.tobytes(), cut
    assert res["tcp_packets"] == 1 and got["payload_bytes"][0, 0] == 100


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason."""
    L = abi.lib()
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    stat = (ctypes.c_uint64 * 64)()
    res = (ctypes.c_uint64 * 4)()
    tsv = (ctypes.c_uint64 * 4)()
    ip, sp, rp, tp = ctypes.addressof(ids), ctypes.addressof(stat), ctypes.addressof(res), ctypes.addressof(tsv)

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    ok_upd = abi.FlowTrackUpdate(tp, 0)

    def update(word, frames, flow_id=ip, flags=0, upd=ok_upd, table=sp, cap=4, result=rp):
        said(L.bt_flow_stat_update_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, flags,
                                          ctypes.byref(upd) if upd is not None else None, table, cap, result, None), word)

    update("null context", good())
    update("null context", good(), upd=abi.FlowTrackUpdate(None, 5))
    update("null frames", None)
    update("null flow_id", good(), flow_id=None)
    update("null upd", good(), upd=None)
    update("null stat", good(), table=None)
    update("null result", good(), result=None)
    update("stat is not 8-byte aligned", good(), table=sp + 4)
    update("flow_id is not 4-byte aligned", good(), flow_id=ip + 1)
    update("ts is not 8-byte aligned", good(), upd=abi.FlowTrackUpdate(tp + 4, 0))
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

    def host(word, base=ctypes.addressof(data), d=ctypes.addressof(desc), flow_id=ip, flags=0, upd=ok_upd, table=sp, cap=4, result=rp):
        said(L.bt_flow_stat_update_host(base, 256, d, 2, flow_id, flags, ctypes.byref(upd) if upd is not None else None, table, cap,
                                        result), word)

    host("null base", base=None)
    host("null base", d=None)
    host("null flow_id", flow_id=None)
    host("null upd", upd=None)
    host("null stat", table=None)
    host("null result", result=None)
    host("stat is not 8-byte aligned", table=sp + 4)
    host("ts is not 8-byte aligned", upd=abi.FlowTrackUpdate(tp + 1, 0))
    host("result is not 8-byte aligned", result=rp + 4)
    host("unknown flag", flags=8)
    assert bytes(stat) == bytes(512) and bytes(res) == bytes(32)

    need = abi.flow_track_side_move_scratch_bytes(4, 128)
    sraw = (ctypes.c_uint8 * (need + 512))()
    scr = (ctypes.addressof(sraw) + 255) & ~255
    remap = (ctypes.c_uint32 * 4)()
    mp = ctypes.addressof(remap)

    def mv(**kw):
        d = dict(side=sp, expired_side=None, remap=mp, result=rp, rec_bytes=128, flow_cap=4, expired_cap=0, reserved=0)
        d.update(kw)
        return abi.FlowSideMove(*d.values())

    def move(word, m, scratch=scr, nbytes=need):
        said(L.bt_flow_track_side_move_device(None, ctypes.byref(m) if m is not None else None, scratch, nbytes, None), word)

    move("null context", mv())
    move("null context", mv(side=None, remap=None, flow_cap=0))
    move("null move", None)
    move("null side", mv(side=None))
    move("null remap", mv(remap=None))
    move("null result", mv(result=None))
    move("side is not 4-byte aligned", mv(side=sp + 2))
    move("expired_side is not 4-byte aligned", mv(expired_side=sp + 1, expired_cap=1))
    move("remap is not 4-byte aligned", mv(remap=mp + 2))
    move("result is not 8-byte aligned", mv(result=rp + 4))
    for rb in (0, 2, 130, 260):
        move("rec_bytes", mv(rec_bytes=rb))
    move("expired_cap != 0 without expired_side", mv(expired_cap=1))
    move("reserved", mv(reserved=1))
    move("null scratch", mv(), scratch=None)
    move("scratch is not 256-byte aligned", mv(), scratch=scr + 64)
    move("scratch_bytes", mv(), nbytes=need - 1)

    def hmove(word, m):
        said(L.bt_flow_track_side_move_host(ctypes.byref(m) if m is not None else None), word)

    hmove("null move", None)
    hmove("null side", mv(side=None))
    hmove("null remap", mv(remap=None))
    hmove("null result", mv(result=None))
    hmove("rec_bytes", mv(rec_bytes=6))
    hmove("expired_cap != 0 without expired_side", mv(expired_cap=2))
    hmove("reserved", mv(reserved=7))
    assert L.bt_flow_track_side_move_host(ctypes.byref(mv())) == 0   # a zero result: nothing moves
    assert bytes(sraw) == bytes(len(sraw)) and bytes(stat) == bytes(512)


def test_flowstat_host_check_builds_and_passes(tmp_path):
    """tools/flowstat_host_check.cpp: the argument checks, the host update, bt_flow_stat_rtt and the host
    side move under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowstat_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowstat_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
