"""CPU: the endpoint table of a flow tracker on the host (bt_flow_track_hosts_host,
include/beatrice_gpu.h) against the restatement in flowhosts_ref.py (a dict group-by over the
records) on crafted tables and on goldens merged by the host tracker, unidirectional and
bidirectional, the ctypes layout of the new structs, the scratch size, and the refusals of the
device call, which need no GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
import flowhosts_ref as fh
import flowtab_ref as ftr
import flowtcp_ref as tr
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
POISON = 0xC7


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert fh.HOST_REC.itemsize == abi.FlowHostRec.itemsize == 128 and re.search(r"typedef struct bt_flow_host_rec \{\s*/\* 128 B", src)
    assert abi.FlowHostRec == fh.HOST_REC
    assert ctypes.sizeof(abi.FlowHostsOpts) == 16 and ctypes.sizeof(abi.FlowHostsOut) == 24
    assert ctypes.sizeof(abi.FlowHostsResult) == 64 and re.search(r"typedef struct bt_flow_hosts_result \{\s*/\* 64 B", src)
    assert (abi.FlowHostsResult.overflow_endpoints.offset, abi.FlowHostsResult.hosts_v6.offset, abi.FlowHostsResult.packets_total.offset,
            abi.FlowHostsResult.bytes_total.offset) == (16, 28, 32, 40)
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_track_hosts_scratch_bytes", "bt_flow_track_hosts_device", "bt_flow_track_hosts_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    for name in ("bt_time_flow_hosts", "bt_time_flow_hosts_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name)
    assert abi.lib().bt_abi_version() == 2


def test_scratch_size_grows_with_flow_cap_and_slots():
    prev = 0
    for cap in (1, 2, 255, 256, 257, 5000, 1 << 20, 1 << 29):
        need = abi.flow_track_hosts_scratch_bytes(cap)
        slots = fh.auto_slots(cap)
        assert need % 256 == 0 and need >= prev and need >= 4 * slots + 8 * cap + 112 * ((cap + 255) // 256), cap
        assert abi.flow_track_hosts_scratch_bytes(cap, slots) == need
        if slots < 1 << 31:
            assert abi.flow_track_hosts_scratch_bytes(cap, 2 * slots) > need
        prev = need
    assert abi.flow_track_hosts_scratch_bytes(1 << 20, 128) < abi.flow_track_hosts_scratch_bytes(1 << 20, 256)
    b = ctypes.c_uint64(0)
    L = abi.lib()
    for cap, slots in ((0, 0), ((1 << 29) + 1, 0), (1 << 31, 128), (64, 100), (64, 64)):
        assert L.bt_flow_track_hosts_scratch_bytes(cap, slots, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT, (cap, slots)
    assert L.bt_flow_track_hosts_scratch_bytes(1, 0, None) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_track_hosts_scratch_bytes((1 << 29) + 1, 1 << 31, ctypes.byref(b)) == 0   # explicit slots lift the auto limit


def host_state(flow_cap, flags, n_flows, recs):
    """A host tracker whose header and records are replaced by crafted ones."""
    t = abi.HostFlowTracker(flow_cap, flags)
    lay = t.layout
    t.state[:128] = np.frombuffer(fh.header(flags, flow_cap, lay["slots"], n_flows), np.uint8)
    t.state[lay["records"]:lay["records"] + 104 * flow_cap] = recs.view(np.uint8).reshape(-1)
    return t


def host_hosts(state, flow_cap, host_cap, slots, tcp, with_ends, want, where):
    """bt_flow_track_hosts_host into poisoned outputs of host_cap records and 2 flow_cap numbers: what is
    expected is there, nothing behind n_written / 2 n_flows is written."""
    hosts = np.full(128 * max(1, host_cap), POISON, np.uint8)
    ends = np.full(max(1, 2 * flow_cap), 0xC7C7C7C7, np.uint32)
    res = abi.FlowHostsResult()
    opts = abi.FlowHostsOpts(slots, host_cap, (ctypes.c_uint32 * 2)(0, 0))
    out = abi.FlowHostsOut(hosts.ctypes.data if host_cap else None, ends.ctypes.data if with_ends else None, ctypes.addressof(res))
    abi._check(abi.lib().bt_flow_track_hosts_host(state.ctypes.data, state.nbytes, ctypes.byref(opts),
                                                  tcp.ctypes.data if tcp is not None else None, ctypes.byref(out)))
    r = res.as_dict()
    if want["overflow"]:
        assert r["overflow_endpoints"] != 0 and (r["status"], r["n_flows"], r["slots"]) == (0, want["n_flows"], want["slots"]), where
        return r, None
    assert r == want["result"], f"{where}: result {r} != {want['result']}"
    nw, nf = r["n_written"], r["n_flows"]
    assert hosts[:128 * nw].tobytes() == want["hosts"].tobytes() and (hosts[128 * nw:] == POISON).all(), f"{where}: hosts"
    if with_ends:
        assert (ends[:2 * nf] == want["endpoint_host"]).all() and (ends[2 * nf:] == 0xC7C7C7C7).all(), f"{where}: endpoint_host"
    else:
        assert (ends == 0xC7C7C7C7).all(), where
    return r, hosts[:128 * nw].view(fh.HOST_REC)


def invariants(hosts, res, recs, with_tcp, where):
    """What holds for every whole table (host_cap >= n_hosts)."""
    assert int(hosts["packets"][:, 0].sum(dtype=np.uint64)) == res["packets_total"] == int(recs["packets"].sum(dtype=np.uint64)), where
    assert int(hosts["bytes"][:, 0].sum(dtype=np.uint64)) == res["bytes_total"] == int(recs["bytes"].sum(dtype=np.uint64)), where
    assert int(hosts["packets"][:, 1].sum(dtype=np.uint64)) == res["packets_total"], where   # every packet is received by a host too
    want = hosts["flows"].sum(axis=1) if with_tcp else 0
    assert (hosts["tcp_state"].sum(axis=1) == want).all(), where
    assert (np.diff(hosts["first_flow"].astype(np.int64)) >= 0).all(), where
    assert int(hosts["flows"].sum()) == 2 * res["n_flows"] and res["hosts_v4"] + res["hosts_v6"] == res["n_hosts"], where


@pytest.mark.parametrize("case", fh.crafted(), ids=lambda c: c[0])
def test_host_form_on_crafted_tables(case):
    name, cap, pairs = case
    n = len(pairs)
    for flags in (ftr.BIDIRECTIONAL, 0):
        recs, tcp = fh.craft(cap, pairs)
        t = host_state(cap, flags, n, recs)
        before = t.state.tobytes(), tcp.tobytes()
        n_hosts = fh.expected(recs[:n], None, flags, 0, 1 << 31)["result"]["n_hosts"]
        exact = max(128, 1 << (n_hosts - 1).bit_length()) if n_hosts else 128
        for host_cap in sorted({0, n_hosts // 2, n_hosts, n_hosts + 3}):
            for slots in (0, exact):
                for side in (tcp, None):
                    where = f"{name} flags={flags} host_cap={host_cap} slots={slots} tcp={side is not None}"
                    want = fh.expected(recs[:n], side, flags, host_cap, slots or fh.auto_slots(cap))
                    r, hosts = host_hosts(t.state, cap, host_cap, slots, side, host_cap % 2 == 0, want, where)
                    if host_cap >= n_hosts:
                        invariants(hosts, r, recs[:n], side is not None, where)
        if n_hosts > 128:   # too few slots: overflow is reported, nothing else is promised
            want = fh.expected(recs[:n], None, flags, 5, 128)
            assert want["overflow"]
            host_hosts(t.state, cap, 5, 128, None, True, want, f"{name}: overflow")
        assert (t.state.tobytes(), tcp.tobytes()) == before   # read-only on both


def test_three_flows_written_out_by_hand():
    """Three flows and what every field of their hosts must be, written out here: a check of the
    restatement both suites compare with, and of bt_flow_track_hosts_host on the same three flows."""
    recs, tcp = np.zeros(3, fkr.FLOW_TRACK_REC), np.zeros(3, tr.TCP_REC)
    a, b, six = fh.v4(0x01020304), fh.v4(0x0A000001), fh.v6(0x01020304 << 96)
    for f, (x, y, klass) in enumerate(((a, b, fh.V4_L4), (b, a, fh.V4), (six, six, fh.V6_L4))):
        recs["key"][f, :2 * len(x)] = np.frombuffer(x + y, np.uint8)
        recs["klass"][f] = klass
    recs["packets"], recs["bytes"] = [[5, 2], [1, 0], [4, 3]], [[500, 200], [60, 0], [(1 << 64) - 1, 3]]
    recs["first_ts"], recs["last_ts"] = [10, 4, 7], [20, 30, 8]
    tcp["flags"], tcp["syn_packets"] = [[0x02, 0x12], [0x04, 0], [0, 0]], [1, 0, 0]
    e = fh.expected(recs, tcp, ftr.BIDIRECTIONAL, 8, 128)
    h = e["hosts"]
    assert e["result"]["n_hosts"] == 3 and e["result"]["hosts_v4"] == 2 and e["result"]["hosts_v6"] == 1
    assert e["endpoint_host"].tolist() == [0, 1, 1, 0, 2, 2]
    assert bytes(h["addr"][0]) == a + bytes(12) and bytes(h["addr"][2]) == six and h["family"].tolist() == [4, 4, 6]
    assert h["flows"].tolist() == [[1, 1], [1, 1], [1, 1]] and h["first_flow"].tolist() == [0, 0, 2]
    assert h["packets"].tolist() == [[5, 3], [3, 5], [7, 7]] and h["bytes"][:2].tolist() == [[500, 260], [260, 500]]
    assert h["bytes"][2].tolist() == [2, 2]                                   # (2^64 - 1) + 3 wraps
    assert h["first_ts"].tolist() == [4, 4, 7] and h["last_ts"].tolist() == [30, 30, 8]
    assert h["tcp_state"][0].tolist() == [0, 0, 1, 0, 0, 1, 0] and h["tcp_state"][2].tolist() == [2, 0, 0, 0, 0, 0, 0]
    assert h["syn_flows"].tolist() == [[1, 1], [1, 1], [0, 0]] and h["syn_packets"].tolist() == [1, 1, 0]
    assert e["result"]["packets_total"] == 15 and e["result"]["bytes_total"] == (760 + (1 << 64) + 2) & fh.M64
    assert fh.expected(recs, None, 0, 1, 128)["hosts"]["tcp_state"].sum() == 0
    assert fh.expected(recs, tcp, 0, 8, 2)["overflow"]
    t = host_state(3, ftr.BIDIRECTIONAL, 3, recs)
    r, hosts = host_hosts(t.state, 3, 8, 0, tcp, True, fh.expected(recs, tcp, ftr.BIDIRECTIONAL, 8, 128), "by hand")
    assert hosts["packets"].tolist() == [[5, 3], [3, 5], [7, 7]] and hosts["flows"].tolist() == [[1, 1]] * 3
    assert hosts["tcp_state"][0].tolist() == [0, 0, 1, 0, 0, 1, 0] and hosts["syn_flows"].tolist() == [[1, 1], [1, 1], [0, 0]]
    assert r["n_hosts"] == 3 and r["packets_total"] == 15


@pytest.mark.parametrize("name", ["c3", "c4", "edge"])
@pytest.mark.parametrize("flags", [0, ftr.BIDIRECTIONAL], ids=["unidirectional", "bidirectional"])
def test_host_tracker_hosts_after_goldens(name, flags):
    """HostFlowTracker.hosts after the golden merged in 1 and in 3 batches (stamped 10 b), with and without the side table."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    keys = fr.key_of_rec(g["rec"], False)
    tcp, fl = tr.tcp_of_rec(g["rec"])
    dirs = tr.directions(*keys, flags)
    n = n0 + n0 // 2   # the golden and half of it again: flows of the first batch come back in the last
    desc, reps = np.resize(g["desc"], n), np.resize(np.arange(n0), n)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    seen = []
    for cuts in (1, 3):
        host, ref = abi.HostFlowTracker(n0, flags), fkr.Tracker(n0, flags)
        want_tcp = np.zeros(n0, tr.TCP_REC)
        bounds = np.linspace(0, n, cuts + 1).astype(int)
        ids = []
        for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            r = reps[lo:hi]
            fid, _ = host.update(g["data"], desc[lo:hi], batch_ts=10 * b)
            wid = ref.update(keys[0][r], keys[1][r], keys[2][r], lens[lo:hi], batch_ts=10 * b)["flow_id"]
            assert (fid == wid).all()
            ids.append(fid)
        recs = ref.records()
        where = f"{name} flags={flags} cuts={cuts}"
        assert len(recs) > 20
        want = fh.expected(recs, None, flags, 2 * n0, fh.auto_slots(n0))
        hosts, ends, res = host.hosts()                       # before the side table exists: the TCP fields are 0
        assert res == want["result"] and hosts.tobytes() == want["hosts"].tobytes() and (ends == want["endpoint_host"]).all(), where
        invariants(hosts, res, recs, False, where)
        for fid, (lo, hi) in zip(ids, zip(bounds[:-1], bounds[1:])):   # no flow has left: the numbers still hold
            r = reps[lo:hi]
            host.tcp_update(g["data"], desc[lo:hi], fid)
            tr.update(want_tcp, fid, tcp[r], fl[r], dirs[r])
        want = fh.expected(recs, want_tcp, flags, 2 * n0, fh.auto_slots(n0))
        hosts, ends, res = host.hosts()
        assert res == want["result"], where
        assert hosts.tobytes() == want["hosts"].tobytes() and (ends == want["endpoint_host"]).all(), where
        invariants(hosts, res, recs, True, where)
        few, _, res_few = host.hosts(host_cap=7, want_endpoints=False)
        assert res_few == dict(want["result"], n_written=7) and few.tobytes() == want["hosts"][:7].tobytes(), where
        seen.append({bytes(h["addr"]) + bytes([h["family"]]): (h["flows"].tolist(), h["packets"].tolist(), h["bytes"].tolist(),
                                                                h["tcp_state"].tolist(), h["syn_packets"]) for h in hosts})
    assert seen[0] == seen[1]   # sums: the same however the capture is cut
    if flags == 0:   # a destination-only host has only received
        only_dst = hosts[hosts["flows"][:, 0] == 0]
        assert len(only_dst) and not only_dst["packets"][:, 0].any() and only_dst["packets"][:, 1].all()


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason, and the unknown state after every other."""
    L = abi.lib()
    lay = abi.flow_track_layout(64)
    raw = (ctypes.c_uint8 * (lay["total"] + 512))()
    st = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_track_hosts_scratch_bytes(64, 1024)
    sraw = (ctypes.c_uint8 * (need + 512))()
    sp = (ctypes.addressof(sraw) + 255) & ~255
    side = (ctypes.c_uint32 * (4 * 64))()
    outs = (ctypes.c_uint64 * 256)()
    res = (ctypes.c_uint64 * 8)()
    xp, op, rp = ctypes.addressof(side), ctypes.addressof(outs), ctypes.addressof(res)

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def opts(slots=0, host_cap=4, r0=0, r1=0):
        return abi.FlowHostsOpts(slots, host_cap, (ctypes.c_uint32 * 2)(r0, r1))

    def out(hosts=op, ends=None, result=rp):
        return abi.FlowHostsOut(hosts, ends, result)

    def dev(word, o=None, u=None, state=st, tcp=None, scratch=sp, nbytes=need, no_opts=False, no_out=False):
        o, u = o or opts(), u or out()
        said(L.bt_flow_track_hosts_device(None, state, None if no_opts else ctypes.byref(o), tcp, scratch, nbytes,
                                          None if no_out else ctypes.byref(u), None), word)

    dev("not an initialised tracker")   # nothing else is wrong: the unknown state, then the null context
    dev("null state", state=None)
    dev("null opts", no_opts=True)
    dev("null out", no_out=True)
    dev("null result", u=out(result=None))
    dev("null scratch", scratch=None)
    dev("state is not 256-byte aligned", state=st + 128)
    dev("scratch is not 256-byte aligned", scratch=sp + 8)
    dev("result is not 8-byte aligned", u=out(result=rp + 4))
    dev("hosts is not 8-byte aligned", u=out(hosts=op + 4))
    dev("tcp is not 4-byte aligned", tcp=xp + 1)
    dev("endpoint_host is not 4-byte aligned", u=out(ends=op + 2))
    dev("slots is not a power of two", o=opts(slots=384))
    dev("slots below 128", o=opts(slots=64))
    dev("reserved", o=opts(r0=1))
    dev("reserved", o=opts(r1=7))
    dev("null hosts with host_cap != 0", u=out(hosts=None))
    dev("not an initialised tracker", o=opts(slots=1024, host_cap=0), tcp=xp, u=out(hosts=None, ends=op))
    dev("not an initialised tracker", nbytes=0)   # the state's flow_cap decides the need: unknown comes first

    def host(word, o=None, u=None, state=st, nbytes=lay["total"], tcp=None, no_opts=False, no_out=False):
        o, u = o or opts(), u or out()
        said(L.bt_flow_track_hosts_host(state, nbytes, None if no_opts else ctypes.byref(o), tcp, None if no_out else ctypes.byref(u)), word)

    host("not an initialised tracker")   # zeros
    assert L.bt_flow_track_init_host(st, lay["total"], ctypes.byref(abi.FlowTrackOpts(0, 64, 0, 0))) == 0
    host("null state", state=None)
    host("state is not 256-byte aligned", state=st + 64)
    host("null opts", no_opts=True)
    host("null out", no_out=True)
    host("null result", u=out(result=None))
    host("result is not 8-byte aligned", u=out(result=rp + 4))
    host("hosts is not 8-byte aligned", u=out(hosts=op + 4))
    host("tcp is not 4-byte aligned", tcp=xp + 2)
    host("endpoint_host is not 4-byte aligned", u=out(ends=op + 1))
    host("slots is not a power of two", o=opts(slots=100))
    host("slots below 128", o=opts(slots=32))
    host("reserved", o=opts(r1=1))
    host("null hosts with host_cap != 0", u=out(hosts=None))
    host("state_bytes below the header's layout", nbytes=lay["total"] - 1)
    assert bytes(outs) == bytes(2048) and bytes(res) == bytes(64) and bytes(sraw) == bytes(len(sraw))
    o, u = opts(), out(ends=op + 1024)
    assert L.bt_flow_track_hosts_host(st, lay["total"], ctypes.byref(o), None, ctypes.byref(u)) == 0
    want = fh.expected(np.zeros(0, fkr.FLOW_TRACK_REC), None, 0, 4, 256)["result"]
    assert abi.FlowHostsResult.from_bytes(bytes(res)).as_dict() == want
    assert bytes(outs) == bytes(2048)   # an empty tracker: no host


def test_flowhosts_host_check_builds_and_passes(tmp_path):
    """tools/flowhosts_host_check.cpp: the layout, the argument checks and the host form against a
    std::map under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowhosts_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowhosts_host_check.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)   # a program that hangs fails here, with its output
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
