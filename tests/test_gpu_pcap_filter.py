"""GPU: bt_pcap_filter (beatrice_amd/csrc/bt_pcap.cpp): a classic pcap file through the compiled
program, chunk by chunk (H2D, filter-only kernel, bt_pass_pack_device with lead = 16, D2H of the
packed bytes). The output must be, byte for byte, the pcap a host loop over the reference's
PacketFilter::applyFilters writes from the passing records: built here in Python from the golden
codes. Record headers carry distinct timestamps and orig_len != incl_len for every third record,
so a rebuilt header would differ from a copied one. Frames sit at whatever offset the records
before them leave: odd ones included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcap_util as pu
from beatrice_amd import abi
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

BT_E_INVALID_ARGUMENT, BT_E_NOT_IMPLEMENTED = 1, 11

# (capture, filter set): none has a host slot. c3 / mixed, a throwing set of each kind, a GPU
# PAYLOAD set on http, everything passes, nothing passes.
CASES = [("c3", "c3"), ("c3", "mixed"), ("c4", "mixed"), ("edge", "mixed"), ("c3", "throw_after"),
         ("edge", "throw_oor"), ("http", "payload_re_11"), ("c3", "empty"), ("edge", "empty"), ("http", "c3"),
         ("edge", "bpf_7")]

_frames = {}


def frames(cap):
    if cap not in _frames:
        _frames[cap] = pu.frames_of(load_golden(cap)[0])
    return _frames[cap]


def _expect(cap, fset, **kw):
    g, man = load_golden(cap)
    code = g[f"code__{fset}"]
    fr = frames(cap)
    want = {"n_in": len(fr), "n_pass": int((code == 0).sum()), "n_reject": int((code == 1).sum()),
            "n_throw": int((code >= 2).sum())}
    return man["filter_sets"][fset], pu.build(fr, **kw), pu.build(fr, keep=code == 0, **kw), want


def _run(ctx, cap, fset, **kw):
    filters, src, want_out, want = _expect(cap, fset, **kw)
    prog = ctx.compile(filters)
    assert all(abi.KINDS[s.kind] != "HOST" for s in prog), f"{cap}/{fset}: a host slot"
    out, res = ctx.pcap_filter(src)
    for k, v in want.items():
        assert res[k] == v, f"{cap}/{fset}: {k} {res[k]} != {v}"
    assert res["out_bytes"] == len(want_out) == len(out), f"{cap}/{fset}: {res['out_bytes']} bytes, want {len(want_out)}"
    if out != want_out:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(want_out, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{cap}/{fset}: {len(bad)} bytes differ, first at {bad[:5]}")
    assert res["truncated"] == 0
    return prog, res


@pytest.mark.parametrize("cap,fset", CASES)
def test_goldens(gpu_ctx, cap, fset):
    prog, res = _run(gpu_ctx, cap, fset)
    if (cap, fset) == ("c3", "c3"):
        assert res["n_pass"] == 356
    if fset.startswith("throw"):
        assert res["n_throw"] > 0 and res["n_pass"] == 0
    if fset == "payload_re_11":
        assert "PAYLOAD" in [abi.KINDS[s.kind] for s in prog] and res["n_pass"] == 2476
    if fset == "empty":
        assert res["n_pass"] == res["n_in"] > 0
    if (cap, fset) in (("http", "c3"), ("edge", "bpf_7")):
        assert res["n_pass"] == 0 and res["out_bytes"] == 24
    # the captures put frames at odd offsets (odd incl_len in front of them)
    if cap in ("edge", "http"):
        _, desc = abi.pcap_index(pu.build(frames(cap)))
        assert ((desc & pu.MASK48) % np.uint64(2) == 1).sum() > 10


def test_small_chunks():
    """c3 (1.4 MB, 4,096 records) in chunks of at most 700 packets and 256 KiB: at least 5 chunks,
    the same bytes; a chunk limit below one maximal record still takes whole records."""
    for pkts, nbytes, least in [(700, 1 << 18, 6), (100000, 100000, 12), (64, 0, 64), (1, 4096, 0)]:
        ctx = abi.Context(0, host_chunk_packets=pkts, host_chunk_bytes=nbytes)
        try:
            cases = [("c3", "c3"), ("c3", "empty")] if pkts > 1 else [("edge", "mixed")]
            for cap, fset in cases:
                _, res = _run(ctx, cap, fset)
                assert res["chunks"] >= max(5, least) if pkts > 1 else res["chunks"] == 319
            if pkts == 700:   # a smaller file after a larger one reuses the staging
                _run(ctx, "edge", "mixed")
                _run(ctx, "c3", "mixed")
        finally:
            ctx.close()


@pytest.mark.parametrize("nanosecond,swapped", [(True, True), (False, True), (True, False)])
def test_other_magics(gpu_ctx, nanosecond, swapped):
    _run(gpu_ctx, "edge", "mixed", nanosecond=nanosecond, swapped=swapped)
    _run(gpu_ctx, "c3", "c3", nanosecond=nanosecond, swapped=swapped)


def test_truncated_input(gpu_ctx):
    g, man = load_golden("edge")
    code = g["code__mixed"]
    fr = frames("edge")
    gpu_ctx.compile(man["filter_sets"]["mixed"])
    whole = pu.build(fr)
    _, desc = abi.pcap_index(whole)
    for k, extra in [(200, 9), (200, 16 + 5), (1, 3), (0, 15)]:
        # the first k records whole, then `extra` bytes of record k
        end = int(desc[k] & pu.MASK48) - 16
        out, res = gpu_ctx.pcap_filter(whole[:end + extra])
        keep = (code == 0) & (np.arange(len(fr)) < k)
        assert out == pu.build(fr, keep=keep), (k, extra)
        assert res["truncated"] == 1 and res["n_in"] == k and res["n_pass"] == int(keep.sum())
    assert int(((code == 0) & (np.arange(len(fr)) < 200)).sum()) > 20


def test_size_query_and_small_output(gpu_ctx):
    filters, src, want_out, want = _expect("c3", "c3")
    gpu_ctx.compile(filters)
    a = np.frombuffer(src, np.uint8)
    L = abi.lib()
    res = abi.PcapResult()
    assert L.bt_pcap_filter(gpu_ctx.h, a.ctypes.data, len(a), None, 0, abi.ctypes.byref(res)) == 0
    assert res.out_bytes == len(want_out) and res.n_pass == want["n_pass"]
    for cap in (len(want_out) - 1, 24, 10, 0):
        out = np.full(len(want_out) + 64, 0xC7, np.uint8)
        res = abi.PcapResult()
        rc = L.bt_pcap_filter(gpu_ctx.h, a.ctypes.data, len(a), out.ctypes.data, cap, abi.ctypes.byref(res))
        assert rc == BT_E_INVALID_ARGUMENT and res.out_bytes == len(want_out), cap
        assert (out[cap:] == 0xC7).all(), f"cap {cap}: bytes written past the capacity"
    out = np.full(len(want_out) + 64, 0xC7, np.uint8)
    assert L.bt_pcap_filter(gpu_ctx.h, a.ctypes.data, len(a), out.ctypes.data, len(want_out), abi.ctypes.byref(res)) == 0
    assert out[:len(want_out)].tobytes() == want_out and (out[len(want_out):] == 0xC7).all()
    # null arguments, and files bt_pcap_index refuses
    assert L.bt_pcap_filter(None, a.ctypes.data, len(a), None, 0, abi.ctypes.byref(res)) == BT_E_INVALID_ARGUMENT
    assert L.bt_pcap_filter(gpu_ctx.h, None, len(a), None, 0, abi.ctypes.byref(res)) == BT_E_INVALID_ARGUMENT
    assert L.bt_pcap_filter(gpu_ctx.h, a.ctypes.data, len(a), None, 0, None) == BT_E_INVALID_ARGUMENT
    with pytest.raises(abi.BtError) as e:
        gpu_ctx.pcap_filter(pu.global_header(linktype=113))
    assert e.value.code == BT_E_NOT_IMPLEMENTED
    out, res = gpu_ctx.pcap_filter(pu.global_header())   # no records: the header alone
    assert out == pu.global_header() and res["n_in"] == 0 and res["out_bytes"] == 24 and res["chunks"] == 0


def test_host_slots_are_refused(gpu_ctx):
    """An installed CUSTOM callback, or a PAYLOAD regex outside the GPU subset, cannot be decided
    on the device: refused before any work instead of a silently different pass set."""
    _, man = load_golden("c3")
    src = pu.build(frames("c3")[:100])
    for filters in (man["filter_sets"]["custom"], [{"type": abi.PAYLOAD, "expr": "(ab)\\1", "priority": 1}]):
        prog = gpu_ctx.compile(filters)
        assert "HOST" in [abi.KINDS[s.kind] for s in prog]
        with pytest.raises(abi.BtError) as e:
            gpu_ctx.pcap_filter(src)
        assert e.value.code == BT_E_NOT_IMPLEMENTED
    gpu_ctx.compile([])


def test_command_line_tool(tmp_path):
    filters, src, want_out, want = _expect("edge", "mixed")
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(src)
    names = {abi.BPF: "bpf", abi.PROTOCOL: "protocol", abi.IP_RANGE: "ip_range", abi.PORT_RANGE: "port_range",
             abi.PAYLOAD: "payload"}
    args = []
    for f in filters:
        if not f.get("enabled", 1):   # a disabled filter takes no part; the tool has no switch for one
            continue
        assert not f.get("custom", 0)
        args += ["--filter", f"{names[f['type']]}:{f.get('expr', '')}:{int(f.get('priority', 0))}"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_filter.py"), "--in", str(fin), "--out",
                        str(fout), *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert fout.read_bytes() == want_out
    for k, v in want.items():
        assert res[k] == v
    assert res["out_bytes"] == len(want_out)
