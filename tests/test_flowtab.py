"""CPU: the flow table on the host (bt_flow_table_host, include/beatrice_gpu.h) against the
restatement in flowtab_ref.py (a dict over (class, key bytes) with the keys from the goldens'
reference-made bt_rec, or from the Python layer walk for crafted frames), the ctypes layout of
the new structs, bt_flow_table_scratch_bytes, and the refusals of bt_flow_table_device, which
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
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
# packets, flows, selected packets without a key (from the goldens' records)
GOLDENS = {"c1": (10000, 10000, 0), "c3": (4096, 4096, 0), "c4": (2048, 2048, 0), "edge": (319, 35, 122),
           "fuzz": (8192, 3541, 4651), "http": (3000, 2190, 253)}


@functools.lru_cache(maxsize=None)
def golden_keys(name, l3_only=False):
    g, _ = load_golden(name)
    return fr.key_of_rec(g["rec"], l3_only)


def golden_want(name, reps, lens, flags=0, select=None, flow_cap=None, slots=0):
    inputs, nbytes, klass = golden_keys(name, bool(flags & ftr.L3_ONLY))
    return ftr.expected(inputs[reps], nbytes[reps], klass[reps], lens, flags, select, flow_cap, slots)


def same(got, want, where=""):
    """(flow_id, flows, result) of abi.flow_table_host against expected()'s dict, whole."""
    flow_id, flows, res = got
    assert res == want["result"], f"{where}: result " + ", ".join(k for k in res if res[k] != want["result"][k])
    assert (flow_id == want["flow_id"]).all(), f"{where}: flow_id at {np.nonzero(flow_id != want['flow_id'])[0][:8]}"
    assert flows.tobytes() == want["flows"].tobytes(), f"{where}: flows"


def host(g, desc, flags=0, select=None, flow_cap=None, slots=0, nbytes=None):
    cap = len(desc) if flow_cap is None else flow_cap
    return abi.flow_table_host(g["data"], desc, abi.FlowTableOpts(flags, slots, cap, 0), select, nbytes)


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_goldens_once_and_repeated(name):
    g, _ = load_golden(name)
    n0, flows0, none0 = GOLDENS[name]
    assert len(g["desc"]) == n0
    for reps_n, flags in ((n0, 0), (3 * n0, 0), (3 * n0, ftr.BIDIRECTIONAL), (2 * n0, ftr.L3_ONLY),
                          (2 * n0, ftr.L3_ONLY | ftr.BIDIRECTIONAL)):
        desc = np.resize(g["desc"], reps_n)
        reps = np.resize(np.arange(n0), reps_n)
        lens = (desc >> np.uint64(48)).astype(np.int64)
        want = golden_want(name, reps, lens, flags)
        if flags == 0:
            assert (want["result"]["n_flows"], want["result"]["none_packets"]) == (flows0, none0 * (reps_n // n0))
            assert (np.diff(want["flows"]["first"].astype(np.int64)) > 0).all()
            assert int(want["flows"]["packets"].sum()) == reps_n - want["result"]["none_packets"]
        same(host(g, desc, flags), want, f"{name} x{reps_n // n0} flags={flags}")


@pytest.mark.parametrize("name", ["edge", "fuzz", "http"])
def test_select_and_flow_cap(name):
    g, _ = load_golden(name)
    n0 = GOLDENS[name][0]
    n = 2 * n0 + 37
    desc = np.resize(g["desc"], n)
    reps = np.resize(np.arange(n0), n)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    rng = np.random.default_rng(n)
    for kind in ("random", "ones", "zeros"):
        bits = {"random": rng.integers(0, 2, n).astype(bool), "ones": np.ones(n, bool), "zeros": np.zeros(n, bool)}[kind]
        sel = fr.pack_bits(bits)
        sel[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # bits at or above n: ignored
        whole = golden_want(name, reps, lens, ftr.BIDIRECTIONAL, sel)
        same(host(g, desc, ftr.BIDIRECTIONAL, sel), whole, f"{name} {kind}")
        nf = whole["result"]["n_flows"]
        for cap in {0, 1, max(nf - 1, 0)}:
            want = golden_want(name, reps, lens, ftr.BIDIRECTIONAL, sel, flow_cap=cap)
            assert want["result"]["n_written"] == min(cap, nf) and want["result"]["n_flows"] == nf
            same(host(g, desc, ftr.BIDIRECTIONAL, sel, flow_cap=cap), want, f"{name} {kind} cap={cap}")
    # a smaller table that still holds every flow gives the same outputs
    nf = GOLDENS[name][1]
    slots = 128
    while slots < nf:
        slots *= 2
    same(host(g, desc, slots=slots), golden_want(name, reps, lens, slots=slots), f"{name} slots={slots}")


def _addr(text):
    import ipaddress
    return ipaddress.ip_address(text).packed


def frame(src, dst, sport=None, dport=None, proto=6, frag=0):
    """Ethernet + IPv4 / IPv6 + TCP (proto 6), UDP (17) or, with sport None, eight bytes of ICMP."""
    s, d = _addr(src), _addr(dst)
    if sport is None:
        proto, l4 = (1 if len(s) == 4 else 58), bytes(8)
    else:
        l4 = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + bytes(16 if proto == 6 else 4)
    if len(s) == 4:
        ip = bytes([0x45, 0]) + (20 + len(l4)).to_bytes(2, "big") + bytes(2) + frag.to_bytes(2, "big") + bytes([64, proto, 0, 0])
        return bytes(12) + b"\x08\x00" + ip + s + d + l4
    return bytes(12) + b"\x86\xdd" + bytes([0x60, 0, 0, 0]) + len(l4).to_bytes(2, "big") + bytes([proto, 64]) + s + d + l4


def pack_frames(frames):
    """(data, desc): the frames back to back, each at an odd offset."""
    data, desc = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)
        desc.append(len(data) | len(f) << 48)
        data += f
    return np.frombuffer(bytes(data), np.uint8), np.array(desc, np.uint64)


CONVERSATIONS = [("10.1.2.3", "10.3.2.1", 40000, 443), ("10.3.2.1", "10.1.2.3", 80, 80), ("10.9.9.9", "10.9.9.9", 5, 4),
                 ("10.9.9.9", "10.9.9.9", 7, 7), ("2001:db8::1", "2001:db8::2", 1000, 53),
                 ("2001:db8:ffff::9", "2001:db8::2", 53, 53), ("fe80::1", "fe80::1", 9, 8)]


def test_bidirectional_conversations():
    """A frame and the same frame with addresses and ports swapped are one flow, each counted in
    its direction: v4 and v6, with and without ports, with equal addresses and equal endpoints."""
    frames = []
    for src, dst, sp, dp in CONVERSATIONS:
        fwd, rev = frame(src, dst, sp, dp), frame(dst, src, dp, sp, )
        frames += [fwd, rev, fwd + bytes(3), frame(src, dst), frame(dst, src)]
    data, desc = pack_frames(frames)
    for flags in (ftr.BIDIRECTIONAL, ftr.BIDIRECTIONAL | ftr.L3_ONLY, 0, ftr.L3_ONLY):
        want = ftr.of_frames(frames, flags)
        got = abi.flow_table_host(data, desc, abi.FlowTableOpts(flags, 0, len(frames), 0))
        same(got, want, f"flags={flags}")
    want = ftr.of_frames(frames, ftr.BIDIRECTIONAL)
    flows = want["flows"]
    # one flow with ports per conversation; the address-only flows of conversations 0 and 1 (the same two hosts) and
    # of 2 and 3 (one host talking to itself) are shared
    assert want["result"]["n_flows"] == len(CONVERSATIONS) + len(CONVERSATIONS) - 2
    for k, (src, dst, sp, dp) in enumerate(CONVERSATIONS):
        f = flows[want["flow_id"][5 * k]]
        a, b = _addr(src) + sp.to_bytes(2, "big"), _addr(dst) + dp.to_bytes(2, "big")
        if a == b:
            assert f["packets"].tolist() == [3, 0]
        elif a < b:
            assert f["packets"].tolist() == [2, 1]
        else:
            assert f["packets"].tolist() == [1, 2]
        assert want["flow_id"][5 * k] == want["flow_id"][5 * k + 1] == want["flow_id"][5 * k + 2]
        assert want["flow_id"][5 * k + 3] == want["flow_id"][5 * k + 4] != want["flow_id"][5 * k]
    one_way = ftr.of_frames(frames, 0)
    assert (one_way["flows"]["packets"][:, 1] == 0).all() and one_way["result"]["n_flows"] > want["result"]["n_flows"]


def test_fragments_land_in_one_address_only_flow():
    a, b = "10.9.9.1", "10.9.9.2"
    frames = [frame(a, b, 5000, 6000, 17, frag=0x2000), frame(a, b, 0x1234, 0x5678, 17, frag=0x2002),
              frame(a, b, 0x9999, 0x1111, 17, frag=0x0004), frame(a, b, 5000, 6000, 17), frame(a, b)]
    data, desc = pack_frames(frames)
    want = ftr.of_frames(frames)
    assert want["flow_id"].tolist() == [0, 0, 0, 1, 0] and want["flows"]["klass"].tolist() == [fr.V4, fr.V4_L4]
    assert want["flows"]["packets"].tolist() == [[4, 0], [1, 0]]
    same(abi.flow_table_host(data, desc, abi.FlowTableOpts(0, 0, 8, 0)), want)


def test_frames_running_past_bytes_read_zeros():
    frames = [frame("10.0.0.1", "10.0.0.2", 1, 2), frame("10.0.0.1", "10.0.0.2", 1, 2), frame("2001:db8::1", "2001:db8::2", 3, 4)]
    data, desc = pack_frames(frames)
    off = int(desc[2] & fr.MASK48)
    for cut in (off + 60, off + 40, off + 13, off - 20, off - 40):
        padded = data.copy()
        padded[cut:] = 0
        cut_frames = [padded[int(d & fr.MASK48):int(d & fr.MASK48) + int(d >> np.uint64(48))].tobytes() for d in desc]
        want = ftr.of_frames(cut_frames)
        same(abi.flow_table_host(data[:cut].copy(), desc, abi.FlowTableOpts(0, 0, 8, 0)), want, f"cut={cut}")


def test_overflow_and_a_full_table():
    frames = [frame("10.0.0.1", "10.0.0.2", 1000 + k, 80) for k in range(129)]
    data, desc = pack_frames(frames)
    fid, flows, res = abi.flow_table_host(data[:], desc[:128], abi.FlowTableOpts(0, 128, 128, 0))
    same((fid, flows, res), ftr.of_frames(frames[:128], slots=128), "128 flows in 128 slots")
    fid, flows, res = abi.flow_table_host(data, desc, abi.FlowTableOpts(0, 128, 129, 0))
    assert res["overflow_packets"] == 1 and fid[128] == abi.FLOW_ID_OVERFLOW and res["slots"] == 128


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowRec.itemsize == 80 and ftr.FLOW_REC == abi.FlowRec
    assert ctypes.sizeof(abi.FlowTableResult) == 72 and ctypes.sizeof(abi.FlowTableOpts) == 16
    assert ctypes.sizeof(abi.FlowTableOut) == 24
    R = abi.FlowTableResult
    assert (R.slots.offset, R.klass_flows.offset, R.none_bytes.offset, R.keyed_bytes.offset) == (24, 32, 56, 64)
    for name, val in (("FLOWTAB_L3_ONLY", "0x1u"), ("FLOWTAB_BIDIRECTIONAL", "0x2u"), ("FLOW_ID_UNSELECTED", "0xFFFFFFFFu"),
                      ("FLOW_ID_NONE", "0xFFFFFFFEu"), ("FLOW_ID_OVERFLOW", "0xFFFFFFFDu")):
        assert getattr(abi, name) == int(val[:-1], 16)
        assert re.search(rf"#define BT_{name}\s+{val}", src)
    assert (ftr.UNSELECTED, ftr.NONE_ID, ftr.OVERFLOW) == (abi.FLOW_ID_UNSELECTED, abi.FLOW_ID_NONE, abi.FLOW_ID_OVERFLOW)
    for name in ("bt_flow_table_scratch_bytes", "bt_flow_table_device", "bt_flow_table_host", "bt_time_flow_table",
                 "bt_time_flow_table_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name)
    assert "bt_flow_table_device" in src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]


def test_scratch_bytes_grow_monotonically():
    ns = [0, 1, 63, 64, 65, 16384, 16385, 1 << 20, (1 << 24) + 1, 1 << 30]
    slots = [128, 256, 4096, 1 << 20, 1 << 31]
    for s in slots:
        sizes = [abi.flow_table_scratch_bytes(n, s) for n in ns]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(x % 256 == 0 for x in sizes)   # 63 and 64 round alike
        assert sizes[0] < sizes[2] < sizes[5] < sizes[6] < sizes[7] < sizes[8] < sizes[9]
    for n in ns:
        sizes = [abi.flow_table_scratch_bytes(n, s) for s in slots]
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
    auto = [abi.flow_table_scratch_bytes(n, 0) for n in ns]
    assert all(b >= a for a, b in zip(auto, auto[1:]))
    for n in ns:
        assert abi.flow_table_scratch_bytes(n, 0) == abi.flow_table_scratch_bytes(n, ftr.auto_slots(n))
    # a word per slot, 80 + 4 bytes a packet, a word per tile and a partial per chunk, at the least
    assert abi.flow_table_scratch_bytes(16385, 128) >= 128 * 4 + 16385 * 84 + 257 * 8 + 2 * 96
    assert abi.flow_table_scratch_bytes(1, 1 << 20) - abi.flow_table_scratch_bytes(1, 128) == 4 * ((1 << 20) - 128)
    L = abi.lib()
    b = ctypes.c_uint64(0)
    for n, s in ((1, 127), (1, 64), (1, 129), (1, 3 << 20), ((1 << 30) + 1, 0)):
        assert L.bt_flow_table_scratch_bytes(n, s, ctypes.byref(b)) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_table_scratch_bytes(1, 128, None) == BT_E_INVALID_ARGUMENT


def test_refusals_need_no_gpu():
    """Every refusal of bt_flow_table_device is decided before the context is looked at: with a
    null context each one is reported by its own reason, and a call with nothing else wrong by
    'null context'."""
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    res = (ctypes.c_uint64 * 9)()   # 72 bytes, 8-byte aligned
    rp = ctypes.addressof(res)
    need = abi.flow_table_scratch_bytes(2, 0)
    raw = (ctypes.c_uint8 * (need + 512))()
    sp = (ctypes.addressof(raw) + 255) & ~255
    L = abi.lib()

    def good():
        return (abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0),
                abi.FlowTableOpts(0, 0, 0, 0), abi.FlowTableOut(None, None, rp))

    def check(word, frames, opts, out, scratch=sp, nbytes=need):
        rc = L.bt_flow_table_device(None, ctypes.byref(frames) if frames is not None else None, None,
                                    ctypes.byref(opts) if opts is not None else None, scratch, nbytes,
                                    ctypes.byref(out) if out is not None else None, None)
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    f, o, out = good()
    check("null context", f, o, out)
    check("null frames", None, o, out)
    check("null opts", f, None, out)
    check("null out", f, o, None)
    check("null result", f, o, abi.FlowTableOut(None, None, None))
    check("result is not 8-byte aligned", f, o, abi.FlowTableOut(None, None, rp + 4))
    check("scratch is not 256-byte aligned", f, o, out, scratch=sp + 128)
    check("null scratch", f, o, out, scratch=None)
    check("below the need", f, o, out, nbytes=need - 1)
    check("below the need", f, abi.FlowTableOpts(0, 256, 0, 0), out)   # more slots than the scratch was sized for
    for flags in (0x4, 0x80000000):
        check("unknown flag", f, abi.FlowTableOpts(flags, 0, 0, 0), out)
    for slots in (3 << 10, 129, 1000):
        check("power of two", f, abi.FlowTableOpts(0, slots, 0, 0), out)
    for slots in (1, 64):
        check("below 128", f, abi.FlowTableOpts(0, slots, 0, 0), out)
    check("null flows", f, abi.FlowTableOpts(0, 0, 1, 0), out)
    for flags in (abi.BATCH_PREFIXES, abi.BATCH_LEAN, abi.BATCH_PREFIXES | abi.BATCH_LEAN):
        f, o, out = good()
        f.flags = flags
        check("BT_BATCH_PREFIXES", f, o, out)
    f, o, out = good()
    f.bytes = 0
    check("bytes == 0", f, o, out)
    f, o, out = good()
    f.desc_format = 2
    check("desc_format", f, o, out)
    f, o, out = good()
    f.base = None
    check("null packet buffer", f, o, out)
    f, o, out = good()
    f.desc, f.stride = None, 0
    check("stride", f, o, out)
    assert bytes(res) == bytes(72) and bytes(raw) == bytes(len(raw))
    # the host call shares the opts checks
    r = abi.FlowTableResult()
    for bad in (abi.FlowTableOpts(4, 0, 0, 0), abi.FlowTableOpts(0, 100, 0, 0), abi.FlowTableOpts(0, 64, 0, 0),
                abi.FlowTableOpts(0, 0, 1, 0)):
        assert L.bt_flow_table_host(ctypes.addressof(data), 256, ctypes.addressof(desc), 2, None, ctypes.byref(bad), None, None,
                                    ctypes.byref(r)) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_table_host(ctypes.addressof(data), 256, ctypes.addressof(desc), 2, None, None, None, None,
                                ctypes.byref(r)) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_table_host(ctypes.addressof(data), 256, ctypes.addressof(desc), 2, None,
                                ctypes.byref(abi.FlowTableOpts(0, 0, 0, 0)), None, None, None) == BT_E_INVALID_ARGUMENT


def test_flowtab_host_check_builds_and_passes(tmp_path):
    """tools/flowtab_host_check.cpp: bt::flowtab_args and bt::flowtab_host under AddressSanitizer
    and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowtab_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowtab_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
