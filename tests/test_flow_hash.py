"""CPU: the RSS flow hash of the fan-out (bt_flow_hash_host, include/beatrice_gpu.h) against the
restatement in flow_ref.py (a bit-serial Toeplitz and the flow-key rule applied to the goldens'
reference-made bt_rec), the published RSS verification vectors, the ctypes layout of the new
structs, and the refusals of bt_flow_fanout_device, which need no GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
from beatrice_amd import abi
from conftest import load_golden
from pcap_util import frames_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1

# source, destination, source port, destination port, hash with ports, hash of the addresses only
V4_VECTORS = [("66.9.149.187", "161.142.100.80", 2794, 1766, 0x51CCC178, 0x323E8FC2),
              ("199.92.111.2", "65.69.140.83", 14230, 4739, 0xC626B0EA, 0xD718262A)]
V6_VECTORS = [("3ffe:2501:200:1fff::7", "3ffe:2501:200:3::1", 2794, 1766, 0x40207D3D, 0x2CC18CD5)]
CLASS_COUNTS = {"c3": [0, 0, 4096, 0, 0], "c4": [0, 0, 1016, 0, 1032], "edge": [122, 46, 114, 24, 13],
                "fuzz": [4651, 1387, 891, 751, 512]}


def _addr(text: str) -> bytes:
    import ipaddress
    return ipaddress.ip_address(text).packed


def tcp_frame(src: str, dst: str, sport: int, dport: int, tags: int = 0) -> bytes:
    """Ethernet (+ 802.1Q tags) + IPv4 or IPv6 + a 20-byte TCP header carrying the tuple."""
    s, d = _addr(src), _addr(dst)
    eth = bytes(12) + b"".join(b"\x81\x00\x00\x07" for _ in range(tags))
    l4 = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + bytes(16)
    if len(s) == 4:
        return eth + b"\x08\x00" + bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + s + d + l4
    return eth + b"\x86\xdd" + bytes([0x60, 0, 0, 0, 0, 20, 6, 64]) + s + d + l4


def test_published_vectors_restatement_and_host():
    for src, dst, sp, dp, full, l3 in V4_VECTORS + V6_VECTORS:
        s, d = _addr(src), _addr(dst)
        ports = sp.to_bytes(2, "big") + dp.to_bytes(2, "big")
        assert fr.toeplitz(fr.DEFAULT_KEY, s + d + ports) == full
        assert fr.toeplitz(fr.DEFAULT_KEY, s + d) == l3
        v6 = len(s) == 16
        for tags in (0, 1, 2):
            f = tcp_frame(src, dst, sp, dp, tags)
            assert fr.walk(f) == (s + d + ports, fr.V6_L4 if v6 else fr.V4_L4)
            h, k, q = abi.flow_hash_host(f, abi.FanoutOpts.make(8))
            assert (h, k, q) == (full, abi.FLOW_V6_L4 if v6 else abi.FLOW_V4_L4, full & 127 & 7)
            h, k, q = abi.flow_hash_host(f, abi.FanoutOpts.make(8, abi.FANOUT_L3_ONLY))
            assert (h, k, q) == (l3, abi.FLOW_V6 if v6 else abi.FLOW_V4, l3 & 127 & 7)


def test_toeplitz_many_equals_the_scalar_form():
    rng = np.random.default_rng(5)
    inputs = rng.integers(0, 256, (64, 36), dtype=np.uint8)
    nbytes = rng.choice([0, 8, 12, 32, 36], 64)
    key = bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    many = fr.toeplitz_many(key, inputs, nbytes)
    for i in range(64):
        assert int(many[i]) == fr.toeplitz(key, bytes(inputs[i, :nbytes[i]]))


def test_symmetric_key_hashes_both_directions_alike():
    sym = abi.FanoutOpts.make(8, abi.FANOUT_KEY_SYMMETRIC)
    dflt = abi.FanoutOpts.make(8)
    for src, dst, sp, dp, _, _ in V4_VECTORS + V6_VECTORS:
        fwd, rev = tcp_frame(src, dst, sp, dp), tcp_frame(dst, src, dp, sp)
        assert abi.flow_hash_host(fwd, sym)[0] == abi.flow_hash_host(rev, sym)[0] != 0
        assert fr.toeplitz(fr.SYMMETRIC_KEY, fr.walk(fwd)[0]) == fr.toeplitz(fr.SYMMETRIC_KEY, fr.walk(rev)[0]) \
            == abi.flow_hash_host(fwd, sym)[0]
    src, dst, sp, dp, full, _ = V4_VECTORS[0]
    assert abi.flow_hash_host(tcp_frame(dst, src, dp, sp), dflt)[0] != full


def _host_all(frames, opts):
    out = np.array([abi.flow_hash_host(f, opts) for f in frames], np.int64).reshape(-1, 3)
    return out[:, 0], out[:, 1], out[:, 2]


@pytest.mark.parametrize("name", ["c1", "c3", "c4", "edge", "fuzz"])
def test_golden_frames_class_hash_and_queue(name):
    """bt_flow_hash_host over the frame bytes against the key rule applied to the reference-made rec."""
    g, _ = load_golden(name)
    frames = frames_of(g)
    user_key = bytes(range(7, 47))
    reta2 = [3 if i % 3 else 5 for i in range(128)]
    cases = [(abi.FanoutOpts.make(8), fr.DEFAULT_KEY, fr.default_reta(8), False),
             (abi.FanoutOpts.make(3, abi.FANOUT_KEY_SYMMETRIC | abi.FANOUT_L3_ONLY), fr.SYMMETRIC_KEY, fr.default_reta(3), True),
             (abi.FanoutOpts.make(64, key=user_key, reta=reta2), user_key, np.array(reta2, np.uint8), False)]
    for opts, key, reta, l3_only in cases:
        inputs, nbytes, klass = fr.key_of_rec(g["rec"], l3_only)
        want_h = fr.toeplitz_many(key, inputs, nbytes)
        h, k, q = _host_all(frames, opts)
        assert (k == klass).all(), np.nonzero(k != klass)[0][:10]
        assert (h == want_h).all(), np.nonzero(h != want_h)[0][:10]
        assert (q == reta[want_h & 127]).all()
        assert (want_h[klass == fr.NONE] == 0).all()
    # the Python walk of the frame bytes agrees with the records as well
    inputs, nbytes, klass = fr.key_of_rec(g["rec"])
    wi, wn, wk = fr.key_of_frames(frames)
    assert (wk == klass).all() and (wn == nbytes).all() and (wi == inputs).all()


@pytest.mark.parametrize("name", sorted(CLASS_COUNTS))
def test_class_counts_of_the_goldens(name):
    g, _ = load_golden(name)
    _, _, klass = fr.key_of_rec(g["rec"])
    assert np.bincount(klass, minlength=5).tolist() == CLASS_COUNTS[name]
    _, k, _ = _host_all(frames_of(g), abi.FanoutOpts.make(8))
    assert np.bincount(k, minlength=5).tolist() == CLASS_COUNTS[name]
    if name == "fuzz":   # fragments whose L4 parsed stay address-keyed
        rec = g["rec"]
        flags = rec[:, 38].astype(np.int64) | rec[:, 39].astype(np.int64) << 8
        frag = (klass == fr.V4) & ((rec[:, 25] & (fr.L_TCP | fr.L_UDP)) != 0) & ((flags & 0x3FFF) != 0)
        assert int(frag.sum()) == 40


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_queue_occupancy_is_not_degenerate(name):
    g, _ = load_golden(name)
    _, _, q = _host_all(frames_of(g), abi.FanoutOpts.make(8))
    counts = np.bincount(q, minlength=8)
    assert counts.min() >= 237 and counts.max() <= 546, counts


def test_short_and_empty_frames():
    o = abi.FanoutOpts.make(4)
    f = tcp_frame("10.0.0.1", "10.0.0.2", 1, 2)
    for n in range(len(f) + 1):
        kb, klass = fr.walk(f[:n])
        assert abi.flow_hash_host(f[:n], o)[:2] == (fr.toeplitz(fr.DEFAULT_KEY, kb), klass), n
    L = abi.lib()
    assert L.bt_flow_hash_host(None, 0, ctypes.byref(o), None, None, None) == 0
    assert L.bt_flow_hash_host(None, 14, ctypes.byref(o), None, None, None) == BT_E_INVALID_ARGUMENT


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert ctypes.sizeof(abi.FanoutResult) == 808 and ctypes.sizeof(abi.FanoutOpts) == 176
    assert ctypes.sizeof(abi.FanoutOut) == 40
    R = abi.FanoutResult
    assert (R.start.offset, R.pad0.offset, R.bytes.offset, R.klass.offset, R.pad1.offset) == (8, 268, 272, 784, 804)
    assert (abi.FanoutOpts.key.offset, abi.FanoutOpts.reta.offset) == (8, 48)
    for name, val in (("KEY_USER", 1), ("KEY_SYMMETRIC", 2), ("RETA_USER", 4), ("L3_ONLY", 8)):
        assert getattr(abi, "FANOUT_" + name) == val
        assert re.search(rf"#define BT_FANOUT_{name}\s+0x{val:x}u", src)
    assert re.search(r"#define BT_FANOUT_MAX_QUEUES 64u", src) and abi.FANOUT_MAX_QUEUES == 64
    assert "BT_FLOW_NONE = 0, BT_FLOW_V4 = 1, BT_FLOW_V4_L4 = 2, BT_FLOW_V6 = 3, BT_FLOW_V6_L4 = 4" in src
    for name in ("bt_flow_fanout_device", "bt_flow_hash_host", "bt_time_fanout"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name)
    r = abi.FanoutResult()
    r.n, r.start[64], r.bytes[63], r.klass[4] = 9, 7, 1 << 40, 3
    d = abi.FanoutResult.from_bytes(bytes(r)).as_dict()
    assert d["n"] == 9 and d["start"][64] == 7 and d["bytes"][63] == 1 << 40 and d["klass"] == [0, 0, 0, 0, 3]
    assert len(d["start"]) == 65 and len(d["bytes"]) == 64


def _refusal(frames, opts, out, ctx=None):
    L = abi.lib()
    rc = L.bt_flow_fanout_device(ctx, ctypes.byref(frames) if frames is not None else None, None,
                                 ctypes.byref(opts) if opts is not None else None,
                                 ctypes.byref(out) if out is not None else None, None)
    return rc, L.bt_last_error().decode()


def test_fanout_refusals_need_no_gpu():
    """Every refusal of bt_flow_fanout_device is decided before the context is looked at: with a
    null context each one is reported by its own reason, and a call with nothing else wrong by
    'null context'."""
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    res = (ctypes.c_uint64 * 101)()   # 808 bytes, 8-byte aligned
    rp = ctypes.addressof(res)

    def good():
        return (abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0),
                abi.FanoutOpts.make(8), abi.FanoutOut(None, None, None, None, rp))

    def check(word, frames, opts, out):
        rc, msg = _refusal(frames, opts, out)
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    f, o, out = good()
    check("null context", f, o, out)
    check("null frames", None, o, out)
    check("null opts", f, None, out)
    check("null out", f, o, None)
    check("null result", f, o, abi.FanoutOut(None, None, None, None, None))
    check("aligned", f, o, abi.FanoutOut(None, None, None, None, rp + 4))
    for flags in (abi.BATCH_PREFIXES, abi.BATCH_PREFIXES | abi.BATCH_LEAN):
        f, o, out = good()
        f.flags = flags
        check("BT_BATCH_PREFIXES", f, o, out)
    for queues in (0, 65, 1 << 31):
        f, o, out = good()
        o.queues = queues
        check("queues", f, o, out)
    f, o, out = good()
    o = abi.FanoutOpts.make(8, reta=[0] * 127 + [8])
    check("reta", f, o, out)
    o = abi.FanoutOpts.make(8, abi.FANOUT_KEY_USER | abi.FANOUT_KEY_SYMMETRIC)
    check("both key flags", f, o, out)
    for flags in (0x10, 0x80000000):
        check("unknown flag", f, abi.FanoutOpts.make(8, flags), out)
    f, o, out = good()
    f.bytes = 0
    check("bytes == 0", f, o, out)
    f, o, out = good()
    f.desc_format = 2
    check("desc_format", f, o, out)
    assert bytes(res) == bytes(808)
    # the opts checks of the host hash are the same ones
    L = abi.lib()
    for bad in (abi.FanoutOpts.make(0), abi.FanoutOpts.make(65), abi.FanoutOpts.make(8, 0x10),
                abi.FanoutOpts.make(8, abi.FANOUT_KEY_USER | abi.FANOUT_KEY_SYMMETRIC), abi.FanoutOpts.make(2, reta=[2] * 128)):
        assert L.bt_flow_hash_host(ctypes.addressof(data), 64, ctypes.byref(bad), None, None, None) == BT_E_INVALID_ARGUMENT
    assert L.bt_flow_hash_host(ctypes.addressof(data), 64, None, None, None, None) == BT_E_INVALID_ARGUMENT


def test_fanout_host_check_builds_and_passes(tmp_path):
    """tools/fanout_host_check.cpp: bt::fanout_args and the host hash under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fanout_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "fanout_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
