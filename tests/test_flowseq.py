"""CPU: a packet's position inside its flow and the per-flow cut-off on the host (bt_flow_seq_host,
include/beatrice_gpu.h) against the restatement in flowseq_ref.py (a plain loop over the packets),
the ctypes layout of the new structs, the scratch size, the table through an expire, and the
refusals of the device call, which need no GPU."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_ref as fr
import flowseq_ref as qr
import flowtab_ref as ftr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
GOLDENS = ["c3", "edge", "http"]
LIMITS = [(0, 0), (1, 0), (3, 0), (0, 1), (0, 200), (3, 200)]


def select_words(kind, n, seed=0):
    """Verdict-layout words with garbage in the last word's bits at or above n (as tests/test_gpu_flowtab.py makes them)."""
    ntiles = (n + 63) // 64
    if kind == "null" or ntiles == 0:
        return None
    rng = np.random.default_rng(seed + n)
    if kind == "ones":
        w = np.full(ntiles, ~np.uint64(0))
    elif kind == "zeros":
        w = np.zeros(ntiles, np.uint64)
    else:
        w = rng.integers(0, 1 << 63, ntiles, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, ntiles, dtype=np.uint64)
    if n % 64:
        w = w.copy()
        w[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
    return w


@functools.lru_cache(maxsize=None)
def source(name, flags=0):
    """A golden repeated 2.5 times: (descriptors, frame lengths, flowtab_ref's flow ids, flows)."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    n = n0 * 5 // 2
    reps = np.resize(np.arange(n0), n)
    desc = g["desc"][reps].astype(np.uint64)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    keys = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
    want = ftr.expected(keys[0][reps], keys[1][reps], keys[2][reps], lens, flags)
    return desc, lens, want["flow_id"], want["result"]["n_flows"]


def both(desc, lens, ids, select, got, want, max_packets=0, max_bytes=0, flags=0, in_place=False):
    """The host form and the restatement on the same inputs: every output, the result and the table."""
    n, nw = len(ids), (len(ids) + 63) // 64
    seq, off = np.full(n, 0x5A5A5A5A, np.uint32), np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = select.copy() if in_place else np.full(nw, 0x5A5A5A5A5A5A5A5A, np.uint64)
    wseq, woff, wout, wres = qr.number(want, ids, lens, select, max_packets, max_bytes, flags)
    res = abi.flow_seq_host(desc, ids, out if in_place else select, got, max_packets, max_bytes, flags, seq=seq, byte_off=off, out_select=out)
    assert res == wres, (res, wres)
    assert (seq == wseq).all() and (off == woff).all() and (out[:nw] == wout).all()
    assert got.tobytes() == want.tobytes()
    return wseq, woff, wout, res


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowSeqRec.itemsize == 16 and qr.SEQ_REC == abi.FlowSeqRec
    assert ctypes.sizeof(abi.FlowSeqOpts) == 32 and ctypes.sizeof(abi.FlowSeqOut) == 24 and ctypes.sizeof(abi.FlowSeqResult) == 64
    assert abi.FlowSeqOpts.flags.offset == 16 and abi.FlowSeqResult.numbered_bytes.offset == 32 and abi.FlowSeqResult.kept_bytes.offset == 40
    assert re.search(r"typedef struct bt_flow_seq_result \{\s*/\* 64 B", src)
    for name, val in (("KEEP_UNKEYED", 1), ("NONE", 0xFFFFFFFF), ("MAX", 0xFFFFFFFE), ("OFF_NONE", (1 << 64) - 1)):
        m = re.search(r"#define BT_FLOW_SEQ_%s\s+(0x[0-9A-Fa-f]+)u" % name, src)
        assert m and int(m.group(1), 16) == val == getattr(abi, "FLOW_SEQ_" + name), name
    assert (qr.KEEP_UNKEYED, qr.SEQ_NONE, qr.SEQ_MAX, qr.OFF_NONE) == (1, 0xFFFFFFFF, 0xFFFFFFFE, (1 << 64) - 1)
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_seq_scratch_bytes", "bt_flow_seq_device", "bt_flow_seq_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    assert "bt_time_flow_seq" in abi.EXPORTS and hasattr(abi.lib(), "bt_time_flow_seq")
    assert abi.lib().bt_abi_version() == 2


def test_scratch_bytes_is_monotone_in_n():
    for cap in (0, 1, 2, 257, 65537, (1 << 24) + 1, 0xFFFFFFFF):
        last = 0
        for n in (0, 1, 63, 64, 65, 16384, 16385, 3 * 16384 + 17, 1 << 20, 1 << 24, 0xFFFFFFFF):
            need = abi.flow_seq_scratch_bytes(n, cap)
            assert need >= last and need % 256 == 0 and need >= 12 * n, (n, cap, need)   # a pair list and the lengths at least
            last = need
    assert abi.lib().bt_flow_seq_scratch_bytes(1, 1, None) == BT_E_INVALID_ARGUMENT


@pytest.mark.parametrize("kind", ["random", "ones", "zeros", "null", "in_place"])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_with_every_kind_of_selection(name, kind):
    """Numbering only, then every limit into the table the calls before left: positions go on across calls."""
    desc, lens, ids, nflows = source(name)
    n = len(desc)
    sel = select_words("random" if kind == "in_place" else kind, n)
    got, want = np.zeros(nflows, abi.FlowSeqRec), np.zeros(nflows, qr.SEQ_REC)
    chosen = fr.select_bits(sel, n).astype(bool)
    for k, (mp, mb) in enumerate(LIMITS):
        wseq, woff, wout, res = both(desc, lens, ids, sel, got, want, mp, mb, flags=k % 2, in_place=kind == "in_place")
        assert res["n"] == n and res["selected"] == int(chosen.sum()) and res["bad_ids"] == 0
        assert res["numbered"] + res["unkeyed"] == res["selected"]
        assert res["flows"] == len(np.unique(ids[chosen & (ids < nflows)]))
        assert res["new_flows"] == (res["flows"] if k == 0 else 0)
        if k == 0:
            assert res["kept"] == res["numbered"] and res["kept_bytes"] == res["numbered_bytes"]
        else:   # every flow met has packets behind it by now
            assert res["kept"] - (res["unkeyed"] if k % 2 else 0) < max(res["numbered"], 1)
            fresh_got, fresh_want = np.zeros(nflows, abi.FlowSeqRec), np.zeros(nflows, qr.SEQ_REC)
            _, _, _, fresh = both(desc, lens, ids, sel, fresh_got, fresh_want, mp, mb, flags=k % 2, in_place=kind == "in_place")
            assert fresh["new_flows"] == fresh["flows"] <= fresh["kept"] - (fresh["unkeyed"] if k % 2 else 0) <= fresh["numbered"]
    assert int(want["packets"].sum()) == len(LIMITS) * int((chosen & (ids < nflows)).sum())


def test_the_cut_off_on_a_crafted_flow():
    """Three flows interleaved: which packets a packet limit, a byte limit and both keep; the packet that
    crosses the byte limit is kept, the next is not."""
    ids = np.array([0, 1, 0, 0, 2, 1, 0, 0xFFFFFFFE, 1, 7, 0], np.uint32)
    lens = np.array([100, 60, 100, 100, 1500, 60, 100, 80, 60, 60, 100], np.int64)
    desc = (lens.astype(np.uint64) << np.uint64(48)) | np.arange(len(ids), dtype=np.uint64) * np.uint64(2048)
    got, want = np.zeros(3, abi.FlowSeqRec), np.zeros(3, qr.SEQ_REC)
    seq, off, out, res = both(desc, lens, ids, None, got, want, max_packets=2)
    assert list(seq) == [0, 0, 1, 2, 0, 1, 3, qr.SEQ_NONE, 2, qr.SEQ_NONE, 4]
    assert list(off[:7]) == [0, 0, 100, 200, 0, 60, 300] and int(off[7]) == qr.OFF_NONE
    assert int(out[0]) == 0b00000110111 and res["kept"] == 5 and res["unkeyed"] == 1 and res["bad_ids"] == 1
    assert abi.decode_flow_seq(seq, off)[6] == (3, 300) and abi.decode_flow_seq(seq, off)[7] is None
    got[:], want[:] = 0, 0
    _, _, out, res = both(desc, lens, ids, None, got, want, max_bytes=150, flags=qr.KEEP_UNKEYED)
    # flow 0 at bytes 0, 100 (kept, crosses), 200 (not); flow 1 at 0, 60, 120; flow 2 at 0; the sentinel is kept
    assert int(out[0]) == 0b00110110111 and res["kept"] == 7 and res["kept_bytes"] == 200 + 180 + 1500
    _, _, out, _ = both(desc, lens, ids, None, got, want, max_packets=6, max_bytes=1 << 40)   # the second call goes on at 5, 3, 1
    assert int(out[0]) == 0b00100110011
    assert [tuple(int(x) for x in r) for r in want] == [(10, 1000), (6, 360), (2, 3000)]


def test_saturation_and_64_bit_limits():
    """seq saturates at SEQ_MAX while the cut-off still decides on the 64-bit count; the sums wrap mod 2^64."""
    ids = np.zeros(5, np.uint32)
    lens = np.full(5, 70000, np.int64)   # a descriptor holds 16 bits: 70000 & 0xFFFF
    desc = (lens.astype(np.uint64) & np.uint64(0xFFFF)) << np.uint64(48)
    lens = lens & 0xFFFF
    start = np.zeros(1, qr.SEQ_REC)
    start["packets"], start["bytes"] = 0xFFFFFFFD, (1 << 40) - 5000
    got, want = start.copy().view(abi.FlowSeqRec), start.copy()
    seq, _, out, res = both(desc, lens, ids, None, got, want, max_packets=0xFFFFFFFF + 1)
    assert list(seq) == [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFE, 0xFFFFFFFE, 0xFFFFFFFE] and int(out[0]) == 0b00111 and res["new_flows"] == 0
    start["packets"], start["bytes"] = (1 << 64) - 2, (1 << 64) - 4465
    got, want = start.copy().view(abi.FlowSeqRec), start.copy()
    _, off, _, res = both(desc, lens, ids, None, got, want)
    assert int(want["packets"][0]) == 3 and int(off[2]) == 4463 and res["new_flows"] == 0


def test_sentinels_bad_ids_and_an_empty_table():
    ids = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 0xFFFFFFFC, 5, 0], np.uint32)
    lens = np.full(len(ids), 64, np.int64)
    desc = np.full(len(ids), 64 << 48, np.uint64)
    for cap in (0, 1, 5, 6):
        got, want = np.zeros(cap, abi.FlowSeqRec), np.zeros(cap, qr.SEQ_REC)
        _, _, _, res = both(desc, lens, ids, None, got, want, max_packets=1, flags=qr.KEEP_UNKEYED)
        assert res["unkeyed"] == 4 and res["bad_ids"] == 3 - (cap > 0) - (cap > 5) and res["kept"] == 4 + res["numbered"]
    got, want = np.zeros(2, abi.FlowSeqRec), np.zeros(2, qr.SEQ_REC)
    _, _, _, res = both(desc[:0], lens[:0], ids[:0], None, got, want)
    assert res["n"] == 0 and res["selected"] == 0


@pytest.mark.parametrize("name", ["http", "edge"])
def test_the_table_goes_through_an_expire_by_the_side_move(name):
    """A host tracker numbers two batches; the sequence table follows an expire by
    bt_flow_track_side_move_host with rec_bytes = 16, and a third batch goes on where its flows were."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    desc = g["desc"].astype(np.uint64)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    host = abi.HostFlowTracker(n0, 0)
    got, want = np.zeros(n0, abi.FlowSeqRec), np.zeros(n0, qr.SEQ_REC)
    half = n0 // 2
    fid1, _ = host.update(g["data"], desc[:half], batch_ts=100)
    both(desc[:half], lens[:half], fid1, None, got, want, max_packets=3)
    fid2, _ = host.update(g["data"], desc[half:], batch_ts=5000)
    both(desc[half:], lens[half:], fid2, None, got, want, max_packets=3)
    before = want.copy()
    _, remap, res = host.expire(5000, 1000, None)
    assert res["n_expired"] > 0 and res["n_flows"] > 0
    gone = abi.flow_track_side_move_host(got, remap, res, res["n_expired"])
    assert len(gone) == res["n_expired"] and gone.dtype.itemsize == 16
    for old in range(res["n_flows_before"]):
        if remap[old] < res["n_flows"]:
            want[remap[old]] = before[old]
    want[res["n_flows"]:] = 0
    assert got.tobytes() == want.tobytes()
    fid3, _ = host.update(g["data"], desc[half:], batch_ts=5001)
    seq, _, _, r3 = both(desc[half:], lens[half:], fid3, None, got, want, max_packets=3)
    keyed = fid3 < n0
    assert r3["new_flows"] == 0 and (seq[keyed] >= 1).all()   # every flow of the second half survived with its count


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason."""
    L = abi.lib()
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 16)()
    res = (ctypes.c_uint64 * 8)()
    seqv = (ctypes.c_uint32 * 4)()
    offv = (ctypes.c_uint64 * 4)()
    words = (ctypes.c_uint64 * 2)()
    raw = (ctypes.c_uint8 * (1 << 16))()
    ip, tp, rp, qp, op, wp = (ctypes.addressof(x) for x in (ids, table, res, seqv, offv, words))
    sp = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_seq_scratch_bytes(2, 4)
    assert 0 < need < (1 << 16) - 256

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def opts(mp=0, mb=0, flags=0, reserved=(0, 0, 0)):
        return abi.FlowSeqOpts(mp, mb, flags, (ctypes.c_uint32 * 3)(*reserved))

    ok_out = abi.FlowSeqOut(qp, op, wp)

    def dev(word, frames, flow_id=ip, select=wp, o=opts(), tab=tp, cap=4, out=ok_out, scratch=sp, nbytes=need, result=rp):
        said(L.bt_flow_seq_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, select,
                                  ctypes.byref(o) if o is not None else None, tab, cap, ctypes.byref(out) if out is not None else None,
                                  scratch, nbytes, result, None), word)

    dev("bt_flow_seq_device: null context", good())
    dev("null context", good(), select=None, out=abi.FlowSeqOut(None, None, None), o=opts(3, 9, 1))
    dev("null frames", None)
    dev("null opts", good(), o=None)
    dev("null out", good(), out=None)
    dev("null result", good(), result=None)
    dev("unknown flag", good(), o=opts(flags=2))
    for k in range(3):
        dev("reserved is not 0", good(), o=opts(reserved=[int(j == k) for j in range(3)]))
    dev("null flow_id", good(), flow_id=None)
    dev("null table", good(), tab=None)
    dev("flow_id is not 4-byte aligned", good(), flow_id=ip + 2)
    dev("seq is not 4-byte aligned", good(), out=abi.FlowSeqOut(qp + 2, op, wp))
    dev("table is not 8-byte aligned", good(), tab=tp + 4)
    dev("select is not 8-byte aligned", good(), select=wp + 4)
    dev("byte_off is not 8-byte aligned", good(), out=abi.FlowSeqOut(qp, op + 4, wp))
    dev("out_select is not 8-byte aligned", good(), out=abi.FlowSeqOut(qp, op, wp + 4))
    dev("result is not 8-byte aligned", good(), result=rp + 4)
    dev("scratch is not 256-byte aligned", good(), scratch=sp + 128)
    dev("null scratch", good(), scratch=None)
    dev("scratch_bytes", good(), nbytes=need - 1)
    for flags in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f = good()
        f.flags = flags
        dev("BT_BATCH_PREFIXES", f)
    f = good()
    f.bytes = 0
    dev("bytes == 0", f)
    f = good()
    f.desc_format = 2
    dev("desc_format", f)
    f = good()
    f.base = None
    dev("null packet buffer", f)
    f = good()
    f.n = 0
    dev("null context", f, flow_id=None, tab=None, cap=0, scratch=None, nbytes=0)   # an empty batch needs none of them

    def host(word, d=ctypes.addressof(desc), flow_id=ip, select=wp, o=opts(), tab=tp, cap=4, out=ok_out, result=rp):
        said(L.bt_flow_seq_host(d, 2, flow_id, select, ctypes.byref(o) if o is not None else None, tab, cap,
                                ctypes.byref(out) if out is not None else None, result), word)

    host("bt_flow_seq_host: null desc", d=None)
    host("null opts", o=None)
    host("null out", out=None)
    host("null result", result=None)
    host("unknown flag", o=opts(flags=0x80000000))
    host("reserved is not 0", o=opts(reserved=(0, 0, 7)))
    host("null flow_id", flow_id=None)
    host("null table", tab=None)
    host("flow_id is not 4-byte aligned", flow_id=ip + 1)
    host("seq is not 4-byte aligned", out=abi.FlowSeqOut(qp + 1, None, None))
    host("table is not 8-byte aligned", tab=tp + 4)
    host("select is not 8-byte aligned", select=wp + 2)
    host("byte_off is not 8-byte aligned", out=abi.FlowSeqOut(None, op + 4, None))
    host("out_select is not 8-byte aligned", out=abi.FlowSeqOut(None, None, wp + 4))
    host("result is not 8-byte aligned", result=rp + 4)
    assert bytes(table) == bytes(128) and bytes(res) == bytes(64) and bytes(words) == bytes(16) and bytes(seqv) == bytes(16)


def test_flowseq_host_check_builds_and_passes(tmp_path):
    """tools/flowseq_host_check.cpp: the argument checks and the host form against a naive per-flow loop over
    a std::map under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowseq_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowseq_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
