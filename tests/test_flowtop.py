"""CPU: the top-K query over a flow tracker on the host (bt_flow_track_top_host,
include/beatrice_gpu.h) against the restatement in flowtop_ref.py (values from the record fields,
np.lexsort over split u64 halves) on crafted states (flowtop_cases.py) and on goldens merged by the
host tracker, the ctypes layout of the new structs, and the refusals of the device call, which need
no GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
import flowtab_ref as ftr
import flowtcp_ref as tr
import flowtop_cases as cases
import flowtop_ref as top
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
POISON = 0xC7


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert ctypes.sizeof(abi.FlowTopResult) == 48 and re.search(r"typedef struct bt_flow_top_result \{\s*/\* 48 B", src)
    assert ctypes.sizeof(abi.FlowTopOpts) == 16 and ctypes.sizeof(abi.FlowTopOut) == 40
    assert (abi.FlowTopResult.n_ties.offset, abi.FlowTopResult.threshold.offset, abi.FlowTopResult.total.offset,
            abi.FlowTopResult.top_total.offset) == (16, 24, 32, 40)
    assert re.search(r"#define BT_FLOW_TOP_MAX_K 4096u", src) and abi.FLOW_TOP_MAX_K == top.MAX_K == 4096
    enum = re.search(r"enum \{ (BT_FLOW_TOP_BYTES = 0.*?) \};", src, flags=re.S).group(1)
    got = {m[0]: int(m[1]) for m in re.findall(r"BT_FLOW_TOP_([A-Z_]+) = (\d)", enum)}
    assert got == {"BYTES": 0, "PACKETS": 1, "DURATION": 2, "TCP_SYN": 3, "TCP_RST": 4}
    assert all(getattr(abi, "FLOW_TOP_" + k) == v == getattr(top, k) for k, v in got.items())
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_track_top_scratch_bytes", "bt_flow_track_top_device", "bt_flow_track_top_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    for name in ("bt_time_flow_top", "bt_time_flow_top_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name)
    assert abi.lib().bt_abi_version() == 2
    for cap in (1, 255, 256, 257, 1 << 20):
        for k in (0, 1, 4096):
            need = abi.flow_track_top_scratch_bytes(cap, k)
            assert need % 256 == 0 and need >= 8 * cap + 8 * 1024 + 12 * k + 48 * ((cap + 255) // 256)
    b = ctypes.c_uint64(0)
    assert abi.lib().bt_flow_track_top_scratch_bytes(0, 1, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert abi.lib().bt_flow_track_top_scratch_bytes(1, 4097, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert abi.lib().bt_flow_track_top_scratch_bytes(1, 1, None) == BT_E_INVALID_ARGUMENT


def host_state(flow_cap, flags, n_flows, recs):
    """A host tracker whose header and records are replaced by crafted ones."""
    t = abi.HostFlowTracker(flow_cap, flags)
    lay = t.layout
    t.state[:128] = np.frombuffer(cases.header(flags, flow_cap, lay["slots"], n_flows), np.uint8)
    t.state[lay["records"]:lay["records"] + 104 * flow_cap] = recs.view(np.uint8).reshape(-1)
    return t


def host_top(state, metric, k, tcp, want, where):
    """bt_flow_track_top_host into poisoned outputs of k entries: the first n_top equal `want`, nothing behind them is written."""
    n = max(1, k)
    ids, vals = np.full(n, 0xC7C7C7C7, np.uint32), np.full(n, 0xC7C7C7C7C7C7C7C7, np.uint64)
    recs, side = np.full(104 * n, POISON, np.uint8), np.full(16 * n, POISON, np.uint8)
    res = abi.FlowTopResult()
    opts = abi.FlowTopOpts(metric, k, (ctypes.c_uint32 * 2)(0, 0))
    out = abi.FlowTopOut(ids.ctypes.data, vals.ctypes.data, recs.ctypes.data, side.ctypes.data if tcp is not None else None,
                         ctypes.addressof(res))
    abi._check(abi.lib().bt_flow_track_top_host(state.ctypes.data, state.nbytes, ctypes.byref(opts),
                                                tcp.ctypes.data if tcp is not None else None, ctypes.byref(out)))
    r = res.as_dict()
    assert r == want["result"], f"{where}: result {r} != {want['result']}"
    nt = r["n_top"]
    assert (ids[:nt] == want["top_id"]).all() and (ids[nt:] == 0xC7C7C7C7).all(), f"{where}: top_id"
    assert (vals[:nt] == want["top_value"]).all() and (vals[nt:] == 0xC7C7C7C7C7C7C7C7).all(), f"{where}: top_value"
    assert recs[:104 * nt].tobytes() == want["top"].tobytes() and (recs[104 * nt:] == POISON).all(), f"{where}: top"
    if tcp is not None:
        assert side[:16 * nt].tobytes() == want["top_tcp"].tobytes() and (side[16 * nt:] == POISON).all(), f"{where}: top_tcp"
    else:
        assert (side == POISON).all()
    return r


@pytest.mark.parametrize("n_flows", cases.N_FLOWS)
def test_host_form_on_crafted_states(n_flows):
    saw_ties = False
    for cap in cases.caps(n_flows):
        for name, metrics, recs, tcp in cases.patterns(n_flows, cap):
            t = host_state(cap, ftr.BIDIRECTIONAL, n_flows, recs)
            before = t.state.tobytes(), tcp.tobytes()
            for metric in metrics:
                for k in cases.ks(n_flows):
                    want = top.expected(metric, k, recs[:n_flows], tcp)
                    side = tcp if metric >= top.TCP_SYN or k % 2 else None   # the side table is optional for the others
                    r = host_top(t.state, metric, k, side, want, f"{name} n={n_flows} cap={cap} metric={metric} k={k}")
                    saw_ties |= r["n_ties"] > 1 and 0 < r["n_top"] < n_flows
            assert (t.state.tobytes(), tcp.tobytes()) == before   # read-only on both
    assert saw_ties or n_flows < 3


def test_the_restatement_orders_values_at_and_above_2_63():
    v = np.array([5, 1 << 63, (1 << 63) - 1, (1 << 64) - 1, 5, 0, 1 << 32, (1 << 32) - 1], np.uint64)
    assert top.order(v).tolist() == [3, 1, 2, 6, 7, 0, 4, 5]
    recs = np.zeros(3, fkr.FLOW_TRACK_REC)
    recs["bytes"] = [[(1 << 64) - 1, 2], [7, 0], [1, 0]]
    recs["first_ts"], recs["last_ts"] = [5, 9, 0], [9, 5, 0]
    assert top.values(top.BYTES, recs).tolist() == [1, 7, 1] and top.values(top.DURATION, recs).tolist() == [4, 0, 0]
    e = top.expected(top.BYTES, 2, recs)
    assert e["top_id"].tolist() == [1, 0] and e["result"]["n_ties"] == 2 and e["result"]["total"] == 9


def test_all_equal_takes_the_first_k_flows_and_ties_end_inside_a_block():
    """What the patterns are there for, stated outright on the restatement both suites compare with."""
    n = 1025
    pats = {name: (recs, tcp) for name, _, recs, tcp in cases.patterns(n, n)}
    e = top.expected(top.BYTES, 300, pats["equal"][0], pats["equal"][1])
    assert e["top_id"].tolist() == list(range(300)) and e["result"]["n_ties"] == n and e["result"]["threshold"] == 1000
    e = top.expected(top.BYTES, 600, pats["two values"][0], pats["two values"][1])
    big = [f for f in range(n) if f % 293 == 3]
    ties = e["top_id"].tolist()[len(big):]
    assert e["top_id"].tolist()[:len(big)] == big and e["result"]["n_ties"] == n - len(big)
    assert ties == [f for f in range(n) if f % 293 != 3][:600 - len(big)] and ties[-1] // 256 == 2 and ties[-1] % 256 not in (0, 255)
    v = top.values(top.PACKETS, pats["highest byte"][0])
    assert (v >= np.uint64(1 << 63)).any() and (v < np.uint64(1 << 56)).any()
    v = top.values(top.BYTES, pats["wrap"][0])
    assert (v < np.uint64(1 << 32)).all() and (pats["wrap"][0]["bytes"][:, 0] > np.uint64(1 << 63)).all()
    r = pats["random"][0]
    assert (r["last_ts"] < r["first_ts"]).any() and (top.values(top.DURATION, r)[r["last_ts"] < r["first_ts"]] == 0).all()


@pytest.mark.parametrize("name", ["c3", "c4", "edge"])
def test_host_tracker_top_after_goldens(name):
    """HostFlowTracker.top after the golden merged in 1 and in 3 batches (stamped 10 b), all five metrics."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    flags = ftr.BIDIRECTIONAL
    keys = fr.key_of_rec(g["rec"], False)
    tcp, fl = tr.tcp_of_rec(g["rec"])
    dirs = tr.directions(*keys, flags)
    n = n0 + n0 // 2   # the golden and half of it again: flows of the first batch come back in the last
    desc, reps = np.resize(g["desc"], n), np.resize(np.arange(n0), n)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    tops = {}
    for cuts in (1, 3):
        host, ref = abi.HostFlowTracker(n0, flags), fkr.Tracker(n0, flags)
        want_tcp = np.zeros(n0, tr.TCP_REC)
        bounds = np.linspace(0, n, cuts + 1).astype(int)
        for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            r = reps[lo:hi]
            fid, _ = host.update(g["data"], desc[lo:hi], batch_ts=10 * b)
            wid = ref.update(keys[0][r], keys[1][r], keys[2][r], lens[lo:hi], batch_ts=10 * b)["flow_id"]
            assert (fid == wid).all()
            host.tcp_update(g["data"], desc[lo:hi], fid)
            tr.update(want_tcp, wid, tcp[r], fl[r], dirs[r])
        recs = ref.records()
        nf = len(recs)
        assert nf > 20
        for metric in top.METRICS:
            for k in (0, 1, 20, nf, 4096):
                want = top.expected(metric, k, recs, want_tcp)
                ids, vals, got, side, res = host.top(metric, k)
                where = f"{name} cuts={cuts} metric={metric} k={k}"
                assert res == want["result"], where
                assert (ids == want["top_id"]).all() and (vals == want["top_value"]).all(), where
                assert got.tobytes() == want["top"].tobytes() and side.tobytes() == want["top_tcp"].tobytes(), where
            if metric in (top.BYTES, top.PACKETS, top.TCP_SYN, top.TCP_RST):   # sums: the same however the capture is cut
                tops.setdefault(metric, []).append((ids.tolist(), vals.tolist()))
        assert cuts == 1 or top.values(top.DURATION, recs).any()
    assert all(a == b for a, b in tops.values())


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason, and the unknown state after every other."""
    L = abi.lib()
    lay = abi.flow_track_layout(64)
    raw = (ctypes.c_uint8 * (lay["total"] + 512))()
    st = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_track_top_scratch_bytes(64, 4096)
    sraw = (ctypes.c_uint8 * (need + 512))()
    sp = (ctypes.addressof(sraw) + 255) & ~255
    side = (ctypes.c_uint32 * (4 * 64))()
    outs = (ctypes.c_uint64 * 64)()
    res = (ctypes.c_uint64 * 6)()
    xp, op, rp = ctypes.addressof(side), ctypes.addressof(outs), ctypes.addressof(res)

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def opts(metric=0, k=4, r0=0, r1=0):
        return abi.FlowTopOpts(metric, k, (ctypes.c_uint32 * 2)(r0, r1))

    def out(top_id=None, top_value=None, recs=None, top_tcp=None, result=rp):
        return abi.FlowTopOut(top_id, top_value, recs, top_tcp, result)

    def dev(word, o=None, u=None, state=st, tcp=None, scratch=sp, nbytes=need, no_opts=False, no_out=False):
        o, u = o or opts(), u or out()
        said(L.bt_flow_track_top_device(None, state, None if no_opts else ctypes.byref(o), tcp, scratch, nbytes,
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
    dev("top_value is not 8-byte aligned", u=out(top_value=op + 4))
    dev("top is not 8-byte aligned", u=out(recs=op + 4))
    dev("top_id is not 4-byte aligned", u=out(top_id=op + 2))
    dev("tcp is not 4-byte aligned", tcp=xp + 1)
    dev("top_tcp is not 4-byte aligned", tcp=xp, u=out(top_tcp=op + 2))
    dev("k above BT_FLOW_TOP_MAX_K", o=opts(k=4097))
    dev("unknown metric", o=opts(metric=5))
    dev("reserved", o=opts(r0=1))
    dev("reserved", o=opts(r1=7))
    dev("TCP metric", o=opts(metric=abi.FLOW_TOP_TCP_SYN))
    dev("TCP metric", o=opts(metric=abi.FLOW_TOP_TCP_RST))
    dev("top_tcp without", u=out(top_tcp=op))
    dev("not an initialised tracker", o=opts(metric=abi.FLOW_TOP_TCP_RST, k=4096), tcp=xp, u=out(op, op, op, op))
    dev("not an initialised tracker", o=opts(k=0))

    def host(word, o=None, u=None, state=st, nbytes=lay["total"], tcp=None, no_opts=False, no_out=False):
        o, u = o or opts(), u or out()
        said(L.bt_flow_track_top_host(state, nbytes, None if no_opts else ctypes.byref(o), tcp, None if no_out else ctypes.byref(u)), word)

    host("not an initialised tracker")   # zeros
    assert L.bt_flow_track_init_host(st, lay["total"], ctypes.byref(abi.FlowTrackOpts(0, 64, 0, 0))) == 0
    host("null state", state=None)
    host("state is not 256-byte aligned", state=st + 64)
    host("null opts", no_opts=True)
    host("null out", no_out=True)
    host("null result", u=out(result=None))
    host("result is not 8-byte aligned", u=out(result=rp + 4))
    host("top is not 8-byte aligned", u=out(recs=op + 4))
    host("k above BT_FLOW_TOP_MAX_K", o=opts(k=5000))
    host("unknown metric", o=opts(metric=9))
    host("reserved", o=opts(r1=1))
    host("TCP metric", o=opts(metric=abi.FLOW_TOP_TCP_SYN))
    host("top_tcp without", u=out(top_tcp=op))
    host("state_bytes below the header's layout", nbytes=lay["total"] - 1)
    assert bytes(outs) == bytes(512) and bytes(res) == bytes(48) and bytes(sraw) == bytes(len(sraw))
    o, u = opts(), out(top_id=op)
    assert L.bt_flow_track_top_host(st, lay["total"], ctypes.byref(o), None, ctypes.byref(u)) == 0
    assert abi.FlowTopResult.from_bytes(bytes(res)).as_dict() == top.expected(0, 4, np.zeros(0, fkr.FLOW_TRACK_REC))["result"]
    assert bytes(outs) == bytes(512)   # an empty tracker: no top


def test_flowtop_host_check_builds_and_passes(tmp_path):
    """tools/flowtop_host_check.cpp: the argument checks, the scratch layout and the host form under
    AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowtop_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowtop_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
