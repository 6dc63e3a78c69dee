"""CPU: per-flow TCP reassembly on the host (bt_flow_reasm_host) behind bt_flow_tcpseq_host, which gives
the offsets: against the restatement in flowreasm_ref.py; for captures without holes, late segments or
differing retransmits against Python's `re` over the generator's true streams; for in-order captures
against bt_flow_stream_host; the named cases by what they must hit; the refusals with a null context."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowreasm_cases as rc  # noqa: E402
import flowreasm_ref as rr  # noqa: E402
import flowstream_ref as sr  # noqa: E402
import flowtcpseq_ref as tr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowstream import lay_out, words_of  # noqa: E402

BIDIR = 2
BT_E_INVALID_ARGUMENT, BT_E_NOT_IMPLEMENTED = 1, 11


def bits_of(words, n):
    return [bool(int(words[i >> 6]) >> (i & 63) & 1) for i in range(n)]


def select_of(rows):
    bits = [r.sel for r in rows]
    sel = None if all(bits) else words_of(bits)
    if sel is not None and len(rows) % 64:
        sel[-1] |= ~np.uint64(0) << np.uint64(len(rows) % 64)   # must be ignored
    return sel


def result_of(res):
    return {k: res[k] for k in rr.RESULT}


def chain_host(calls, cap, blob, flags=BIDIR, alias=None):
    """Every call through bt_flow_tcpseq_host, then bt_flow_reasm_host and the restatement from the same
    offsets. alias: None, "hit" or "rest" written in place of select. Returns (the restatement, [(hit bits,
    rest bits, result)])."""
    model = rr.Reasm(cap, blob, flags)
    seq_tab, tab = np.zeros(cap, abi.FlowTcpseqRec), np.zeros(cap, abi.FlowReasmRec)
    out = []
    for k, rows in enumerate(calls):
        n, nw = len(rows), (len(rows) + 63) // 64
        frames, ids = [r.frame for r in rows], np.array([r.flow for r in rows], np.uint32)
        data, desc = lay_out(frames)
        sel = select_of(rows)
        if alias and sel is None:
            sel = words_of([True] * n)
        off = np.full(n, 7, np.int64)
        abi.flow_tcpseq_host(data, desc, ids, sel, flags, seq_tab, off=off)
        want_hit, want_rest, want_res = model.batch(frames, ids, off, sel)
        hit, rest = np.full(nw, 0xDEADBEEF, np.uint64), np.full(nw, 0xDEADBEEF, np.uint64)
        if alias == "hit":
            hit = sel.copy()
            res = abi.flow_reasm_host(data, desc, ids, hit, off, flags, blob, tab, hit=hit, rest=rest)
        elif alias == "rest":
            rest = sel.copy()
            res = abi.flow_reasm_host(data, desc, ids, rest, off, flags, blob, tab, hit=hit, rest=rest)
        else:
            res = abi.flow_reasm_host(data, desc, ids, sel, off, flags, blob, tab, hit=hit, rest=rest)
        assert res["reserved0"] == 0 and res["reserved1"] == 0
        assert result_of(res) == want_res, f"call {k}: result {result_of(res)} != {want_res}"
        bad = [i for i in range(n) if (int(hit[i >> 6]) ^ int(want_hit[i >> 6])) >> (i & 63) & 1]
        assert not bad and (hit == want_hit).all(), f"call {k}: hit differs at packets {bad[:8]}"
        assert (rest == want_rest).all(), f"call {k}: rest"
        assert tab.tobytes() == model.table.tobytes(), f"call {k}: table"
        out.append((bits_of(hit, n), bits_of(rest, n), want_res))
    return model, out


def arrival_hits(rows, pattern, blob, select=None, cap=None):
    """The arrival-order matcher's restatement over one call's rows: hit bits."""
    cap = 1 + max(r.flow for r in rows if r.flow < 1 << 30) if cap is None else cap
    hit, _ = sr.Streams(cap, pattern, blob, BIDIR).batch([r.frame for r in rows], [r.flow for r in rows], select)
    return bits_of(hit, len(rows))


def models(rows, blob, cap=1):
    """One call through the two restatements: (tcpseq's out_select bits, reasm's hit bits)."""
    frames, ids = [r.frame for r in rows], [r.flow for r in rows]
    _, off, osel, _ = tr.Space(cap, BIDIR).batch(frames, ids)
    hit, _, _ = rr.Reasm(cap, blob, BIDIR).batch(frames, ids, off)
    return osel, bits_of(hit, len(rows))


def test_the_cases_are_not_vacuous():
    """On the models alone: arrival order misses what reassembly hits; arrival order with the retransmits
    left in hits falsely; the selection without the OLD segments loses a hole-filler that reassembly uses."""
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    c = rc.Conn(0, 1000, 5000)
    swapped = [rc.seg(c, 0, 6, b"LOdef"), rc.seg(c, 0, 0, b"abcHEL")]
    assert arrival_hits(swapped, rc.PATTERN, blob) == [False, False] and models(swapped, blob)[1] == [True, False]
    resent = [rc.seg(c, 0, 0, b"HEL"), rc.seg(c, 0, 2, b"L"), rc.seg(c, 0, 3, b"O")]   # the true stream is HELO
    assert arrival_hits(resent, rc.PATTERN, blob) == [False, False, True] and models(resent, blob)[1] == [False] * 3
    filler = [rc.seg(c, 0, 0, b"xHE"), rc.seg(c, 0, 4, b"LOy"), rc.seg(c, 0, 3, b"L")]
    osel, hits = models(filler, blob)
    assert bits_of(osel, 3) == [True, True, False]   # the filler is OLD to the sequence call
    assert arrival_hits(filler, rc.PATTERN, blob, osel) == [False] * 3 and hits == [False, True, False]


@pytest.mark.parametrize("flags", [BIDIR, 0])
def test_the_named_cases(flags):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, cap, expect = rc.crafted()
    model, out = chain_host(calls, cap, blob, flags)
    if not flags:
        return   # without directions the two sides of a connection share a sequence space: the restatement alone
    for rows, (hit, rest, _) in zip(calls, out):
        for i, r in enumerate(rows):
            if r.hit is not None:
                assert hit[i] == r.hit, (r.flow, i, r.data)
    table = model.table
    for f, fields in expect.items():
        for (d, name), v in fields.items():
            assert int(table[f]["d"][d][name]) == v, (f, d, name, int(table[f]["d"][d][name]), v)
    last = calls[0][-5:]   # what is not placed: the UDP packet, the ARP frame and the pure ACK
    assert [r.key is None for r in last] == [False, True, True, True, False] and out[0][1][-5:] == [False, True, True, True, False]
    assert out[1][2]["unkeyed"] == 4 and out[1][2]["bad_ids"] == 2 and out[1][2]["far_packets"] == 1 and out[1][2]["late_packets"] == 1
    assert out[1][1][-7:-1] == [True] * 6 and not out[1][1][-1]   # sentinels and bad ids were not placed; unselected is not in rest


def test_a_64_position_pattern_whose_tail_spans_many_tiny_segments():
    blob, info = abi.flow_stream_compile(rc.LONG)
    assert info["positions"] == 64 and info["tail"] == 63
    calls, cap = rc.long_pattern()
    _, out = chain_host(calls, cap, blob)
    want = [r.dstart <= 65 < r.dstart + len(r.data) for r in calls[0]]   # the packet that holds the match's last byte
    assert out[0][0] == want and sum(want) == 1 and out[0][2]["holes"] == 0


def oracle(calls, truth, pattern):
    """From the true streams alone: per call the packets a match must end in. A match end belongs to the
    first segment, in (offset, index) order inside the earliest call, that covers its byte."""
    rx = re.compile(pattern.encode("latin-1"), re.DOTALL)
    want = [[False] * len(rows) for rows in calls]
    for key, s in truth.items():
        ends = {e - 1 for e in range(1, len(s) + 1) if any(rx.fullmatch(s, b, e) for b in range(max(0, e - 64), e))}
        done = 0   # every byte below it has its packet
        for k, rows in enumerate(calls):
            mine = sorted((r.dstart - 1, i, len(r.data)) for i, r in enumerate(rows) if r.key == key and r.data)
            for a, i, ln in mine:
                if any(x in ends for x in range(max(a, done), a + ln)):
                    want[k][i] = True
                done = max(done, a + ln)
    return want


@pytest.mark.parametrize("seed", range(6))
def test_clean_captures_against_re_over_the_true_streams(seed):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, truth = rc.random_calls(seed, nflows=3, nbytes=500 + 97 * seed, ncalls=1 + seed % 3, clean=True)
    model, out = chain_host(calls, 3, blob)
    assert [o[0] for o in out] == oracle(calls, truth, rc.PATTERN)
    assert sum(o[2]["holes"] + o[2]["late_packets"] + o[2]["far_packets"] for o in out) == 0
    assert sum(o[2]["dup_packets"] for o in out) > 0 and sum(o[2]["hit_packets"] for o in out) > 3
    table = model.table
    for (f, d), s in truth.items():
        first = [r for rows in calls for r in rows if r.key == (f, d)][0]   # the sequence call's origin
        assert int(table[f]["d"][d]["next"]) == 1 + len(s) - first.off


@pytest.mark.parametrize("seed", range(4))
def test_disturbed_captures_against_the_restatement(seed):
    blob, _ = abi.flow_stream_compile("GET|POST" if seed % 2 else rc.PATTERN)
    calls, _ = rc.random_calls(100 + seed, nflows=4, nbytes=700, ncalls=3, clean=False)
    _, out = chain_host(calls, 4, blob, BIDIR if seed < 3 else 0)
    assert sum(o[2]["holes"] for o in out) > 0 and sum(o[2]["late_packets"] for o in out) > 0


def test_in_order_captures_against_the_arrival_order_matcher():
    """Every stream in order, no duplicates: hit equals bt_flow_stream_host's on the TCP packets, word for
    word, and rest is exactly the other packets."""
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls = rc.in_order()
    rows = calls[0]
    _, out = chain_host(calls, 3, blob)
    is_tcp = [r.key is not None for r in rows]
    assert out[0][1] == [not t for t in is_tcp] and not all(is_tcp)
    data, desc = lay_out([r.frame for r in rows])
    hit = np.zeros((len(rows) + 63) // 64, np.uint64)
    abi.flow_stream_host(data, desc, np.array([r.flow for r in rows], np.uint32), words_of(is_tcp), BIDIR, blob, np.zeros(3, abi.FlowStreamRec), hit=hit)
    assert bits_of(hit, len(rows)) == out[0][0] and sum(out[0][0]) > 3


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_at_tile_edges(n, cap):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, _ = rc.random_calls(n + cap, nflows=cap, nbytes=200, ncalls=1, clean=False)
    rows = calls[0]
    while 0 < len(rows) < 2 * n:
        rows = rows + [r.again_data() for r in rows]
    first, second = rows[:n], rows[n:2 * n]
    _, out = chain_host([first, second], cap, blob)
    assert out[0][2]["n"] == n and out[1][2]["n"] == n


@pytest.mark.parametrize("alias", ["hit", "rest"])
def test_hit_and_rest_in_place_of_select(alias):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, cap, _ = rc.crafted()
    _, plain = chain_host(calls, cap, blob)
    _, same = chain_host(calls, cap, blob, alias=alias)
    assert plain == same


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at, each by its own reason, the null context last."""
    L = abi.lib()
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 64)()
    res = (ctypes.c_uint64 * 8)()
    words = (ctypes.c_uint64 * 2)()
    more = (ctypes.c_uint64 * 2)()
    offs = (ctypes.c_int64 * 4)()
    raw = (ctypes.c_uint8 * (1 << 17))()
    ip, tp, rp, wp, mp, op, bp = (ctypes.addressof(x) for x in (ids, table, res, words, more, offs, data))
    pp = blob.ctypes.data
    sp = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_reasm_scratch_bytes(2, 4)
    assert 0 < need <= (1 << 17) - 256 and abi.flow_reasm_scratch_bytes(0, 0) >= 256

    def said(rc_, word, code=BT_E_INVALID_ARGUMENT):
        msg = L.bt_last_error().decode()
        assert rc_ == code and word in msg, (word, rc_, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def out_of(hit=wp, rest=mp, result=rp, reserved=(0, 0)):
        return abi.FlowReasmOut(hit, rest, result, (ctypes.c_uint64 * 2)(*reserved))

    def dev(word, frames, flow_id=ip, select=wp, off=op, flags=0, pat=pp, pdev=bp, pbytes=len(blob), tab=tp, cap=4, scratch=sp, nbytes=need,
            out=out_of(), code=BT_E_INVALID_ARGUMENT):
        said(L.bt_flow_reasm_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, select, off, flags, pat, pdev, pbytes,
                                    tab, cap, scratch, nbytes, ctypes.byref(out) if out is not None else None, None), word, code)

    dev("bt_flow_reasm_device: null context", good())
    dev("null context", good(), select=None, out=out_of(hit=None, rest=None), flags=3)
    dev("null frames", None)
    dev("null out", good(), out=None)
    dev("null result", good(), out=out_of(result=None))
    dev("unknown flag", good(), flags=4)
    for k in range(2):
        dev("reserved is not 0", good(), out=out_of(reserved=[int(j == k) for j in range(2)]))
    dev("null flow_id", good(), flow_id=None)
    dev("null off", good(), off=None)
    dev("null table", good(), tab=None)
    dev("flow_id is not 4-byte aligned", good(), flow_id=ip + 2)
    dev("table is not 8-byte aligned", good(), tab=tp + 4)
    dev("select is not 8-byte aligned", good(), select=wp + 4)
    dev("off is not 8-byte aligned", good(), off=op + 4)
    dev("hit is not 8-byte aligned", good(), out=out_of(hit=wp + 4))
    dev("rest is not 8-byte aligned", good(), out=out_of(rest=mp + 4))
    dev("result is not 8-byte aligned", good(), out=out_of(result=rp + 4))
    dev("hit and rest are one", good(), out=out_of(rest=wp))
    dev("flow_cap above 2^31", good(), cap=(1 << 31) + 1)
    dev("null pattern_device", good(), pdev=None)
    dev("pattern_device is not 8-byte aligned", good(), pdev=bp + 4)
    dev("scratch is not 256-byte aligned", good(), scratch=sp + 8)
    for flag in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f = good()
        f.flags = flag
        dev("BT_BATCH_PREFIXES", f)
    dev("null pattern", good(), pat=None)
    dev("pattern_bytes below", good(), pbytes=40)
    dfa, _size = np.zeros(1 << 16, np.uint8), ctypes.c_uint32(0)
    assert L.bt_payload_dfa_compile_ex(b"(ab)+c", 0, dfa.ctypes.data, len(dfa), ctypes.byref(_size)) == 0
    dev("unbounded memory", good(), pat=dfa.ctypes.data, pbytes=_size.value, code=BT_E_NOT_IMPLEMENTED)
    dev("null scratch", good(), scratch=None)
    dev("scratch_bytes", good(), nbytes=need - 1)
    f = good()
    f.n = 0
    dev("null context", f, flow_id=None, off=None, tab=None, cap=0, scratch=None, nbytes=0)   # an empty batch needs none of them

    def host(word, base=bp, d=ctypes.addressof(desc), flow_id=ip, select=wp, off=op, flags=0, pat=pp, pbytes=len(blob), tab=tp, cap=4,
             out=out_of(), code=BT_E_INVALID_ARGUMENT):
        said(L.bt_flow_reasm_host(base, 256, d, 2, flow_id, select, off, flags, pat, pbytes, tab, cap,
                                  ctypes.byref(out) if out is not None else None), word, code)

    host("bt_flow_reasm_host: null base / desc", d=None)
    host("null out", out=None)
    host("null result", out=out_of(result=None))
    host("unknown flag", flags=0x80000000)
    host("reserved is not 0", out=out_of(reserved=(0, 7)))
    host("null flow_id", flow_id=None)
    host("null off", off=None)
    host("null table", tab=None)
    host("off is not 8-byte aligned", off=op + 4)
    host("rest is not 8-byte aligned", out=out_of(rest=mp + 2))
    host("hit and rest are one", out=out_of(hit=mp))
    host("flow_cap above 2^31", cap=(1 << 31) + 1)
    host("null pattern", pat=None)
    host("unbounded memory", pat=dfa.ctypes.data, pbytes=_size.value, code=BT_E_NOT_IMPLEMENTED)


def test_flowreasm_host_check_builds_and_passes(tmp_path):
    """tools/flowreasm_host_check.cpp: the argument checks and the chain of the two host forms against an oracle on
    true 64-bit positions and std::regex, under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    program."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowreasm_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "beatrice_amd", "csrc"),
                    os.path.join(root, "tools", "flowreasm_host_check.cpp"), os.path.join(root, "beatrice_amd", "csrc", "bt_regex_dfa.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks hold" in r.stdout, r.stdout + r.stderr


def test_an_empty_batch_needs_no_offsets():
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    tab = np.zeros(2, abi.FlowReasmRec)
    for off in (None, np.zeros(0, np.int64)):
        res = abi.flow_reasm_host(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), None, off, BIDIR, blob, tab)
        assert result_of(res) == {k: 0 for k in rr.RESULT} and not tab.tobytes().strip(b"\0")
