"""CPU: the per-flow mark side table and the selection built from it on the host
(bt_flow_mark_update_host, bt_flow_mark_select_host, include/beatrice_gpu.h) against the restatement
in flowmark_ref.py (flow numbers through flow_ref and flowtab_ref, lengths from the descriptors), the
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
import flowmark_ref as mr
import flowtab_ref as ftr
import flowtrack_ref as fkr
from beatrice_amd import abi
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
GOLDENS = ["c3", "edge", "http"]
U64_MAX = (1 << 64) - 1
OPS = (mr.SET, mr.AND, mr.OR, mr.ANDNOT)


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


def stamps(n, seed):
    """Per-packet timestamps that are not in order."""
    return np.uint64(1000) + np.random.default_rng(seed).integers(0, 5000, n).astype(np.uint64)


def both_update(desc, lens, ids, hit, mark, got, want, ts=None, batch_ts=0):
    res = abi.flow_mark_update_host(desc, ids, hit, mark, got, ts=ts, batch_ts=batch_ts)
    wres = mr.update(want, ids, lens, hit, mark, batch_ts if ts is None else ts)
    assert res == wres, (res, wres)
    assert got.tobytes() == want.tobytes()
    return res


def test_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert abi.FlowMarkRec.itemsize == 32 and mr.MARK_REC == abi.FlowMarkRec
    assert re.search(r"typedef struct bt_flow_mark_rec \{\s*/\* 32 B", src)
    assert ctypes.sizeof(abi.FlowMarkResult) == 32 and re.search(r"typedef struct bt_flow_mark_result \{\s*/\* 32 B", src)
    assert ctypes.sizeof(abi.FlowMarkSelectResult) == 32 and ctypes.sizeof(abi.FlowMarkSelectOpts) == 16
    assert ctypes.sizeof(abi.FlowMarkUpdate) == 24 and abi.FlowMarkUpdate.ts.offset == 8 and abi.FlowMarkUpdate.batch_ts.offset == 16
    assert abi.FlowMarkResult.new_marked_flows.offset == 20 and abi.FlowMarkSelectResult.bad_ids.offset == 12
    enum = re.search(r"enum \{ (BT_FLOW_MARK_SET = 0.*?) \};", src, flags=re.S).group(1)
    got = {m[0]: int(m[1]) for m in re.findall(r"BT_FLOW_MARK_([A-Z]+) = (\d+)", enum)}
    assert got == {"SET": 0, "AND": 1, "OR": 2, "ANDNOT": 3}
    assert all(getattr(abi, "FLOW_MARK_" + k) == v == getattr(mr, k) for k, v in got.items())
    assert re.search(r"#define BT_FLOW_MARK_ALL_BITS 0x1u", src) and abi.FLOW_MARK_ALL_BITS == 1 == mr.ALL_BITS
    history = src[src.index("ABI history"):src.index("#define BT_ABI_VERSION")]
    for name in ("bt_flow_mark_update_device", "bt_flow_mark_update_host", "bt_flow_mark_select_device", "bt_flow_mark_select_host"):
        assert name in abi.EXPORTS and hasattr(abi.lib(), name) and name in history, name
    assert "bt_time_flow_mark" in abi.EXPORTS and hasattr(abi.lib(), "bt_time_flow_mark")
    assert abi.lib().bt_abi_version() == 2


@pytest.mark.parametrize("kind", ["random", "ones", "zeros", "null"])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_with_every_kind_of_hit_words(name, kind):
    """Unordered per-packet stamps, then a second update with another mark bit and the batch's stamp
    into the first one's table: new_marked_flows of both calls, and of a third that repeats the first."""
    desc, lens, ids, nflows = source(name)
    n = len(desc)
    hit = select_words(kind, n)
    got, want = np.zeros(nflows, abi.FlowMarkRec), np.zeros(nflows, mr.MARK_REC)
    r1 = both_update(desc, lens, ids, hit, 0x4, got, want, ts=stamps(n, 1))
    hit_flows = len(np.unique(ids[fr.select_bits(hit, n) & (ids < nflows)]))
    assert r1["new_marked_flows"] == hit_flows and r1["n"] == n and r1["bad_ids"] == 0
    if kind == "zeros":
        assert r1["hit_packets"] == 0 and not got.tobytes().strip(b"\0")
    else:
        assert 0 < hit_flows <= nflows and r1["marked_packets"] + r1["unkeyed_hits"] == r1["hit_packets"] > 0
        assert int(want["hit_bytes"].sum()) == int(np.minimum(lens, 65535)[fr.select_bits(hit, n) & (ids < nflows)].sum())
    hit2 = select_words("random", n, seed=7)
    r2 = both_update(desc, lens, ids, hit2, 0x80000001, got, want, batch_ts=77)
    assert r2["new_marked_flows"] == len(np.unique(ids[fr.select_bits(hit2, n) & (ids < nflows)])) > 0
    r3 = both_update(desc, lens, ids, hit, 0x4, got, want, ts=stamps(n, 2))
    assert r3["new_marked_flows"] == 0
    # a mark of two bits, one of them there already: the flows that lack the other are new
    r4 = both_update(desc, lens, ids, None, 0x6, got, want, batch_ts=U64_MAX)
    assert r4["new_marked_flows"] == nflows and r4["hit_packets"] == n
    assert ((want["marks"] & 0x6) == 0x6).all()


def test_the_extreme_stamps():
    """2^64 - 1 is a last stamp but reads as no first stamp; 0 is a first stamp (~0) and no last one."""
    desc = np.array([60 << 48, 70 << 48, 80 << 48, 90 << 48], np.uint64)
    lens = [60, 70, 80, 90]
    got, want = np.zeros(3, abi.FlowMarkRec), np.zeros(3, mr.MARK_REC)
    both_update(desc, lens, [0, 0, 1, 2], None, 1, got, want, ts=np.array([U64_MAX, 5, 0, U64_MAX], np.uint64))
    d = [abi.decode_flow_mark(r) for r in got]
    assert d[0] == {"marks": 1, "hit_packets": 2, "hit_bytes": 130, "first_hit_ts": 5, "last_hit_ts": U64_MAX}
    assert d[1]["first_hit_ts"] == 0 and d[1]["last_hit_ts"] == 0 and int(got["first_hit_ts_c"][1]) == U64_MAX
    assert d[2]["first_hit_ts"] is None and d[2]["last_hit_ts"] == U64_MAX
    both_update(desc, lens, [2, 2, 2, 2], None, 1, got, want, batch_ts=9)
    assert abi.decode_flow_mark(got[2])["first_hit_ts"] == 9 and int(got["hit_packets"][2]) == 5


def test_sentinels_bad_ids_and_an_empty_table():
    """Ids are looked at for hit packets only; sentinels are unkeyed hits, other ids at or past flow_cap bad ids."""
    ids = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 0xFFFFFFFC, 5, 6, 4] + [4] * 60, np.uint32)
    n = len(ids)
    desc = (np.arange(n, dtype=np.uint64) * np.uint64(64)) | (np.uint64(54) + np.arange(n, dtype=np.uint64) % np.uint64(11)) << np.uint64(48)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    got, want = np.zeros(5, abi.FlowMarkRec), np.zeros(5, mr.MARK_REC)
    r = both_update(desc, lens, ids, None, 2, got, want, batch_ts=3)
    assert (r["hit_packets"], r["marked_packets"], r["unkeyed_hits"], r["bad_ids"], r["new_marked_flows"]) == (70, 63, 4, 3, 3)
    hit = fr.pack_bits(np.arange(n) % 2 == 0)   # the even packets: ids 0, EXPIRED .. at 2, 4; 0xFFFFFFFC at 6; 6 at 8
    got, want = np.zeros(5, abi.FlowMarkRec), np.zeros(5, mr.MARK_REC)
    r = both_update(desc, lens, ids, hit, 2, got, want, batch_ts=3)
    assert (r["hit_packets"], r["unkeyed_hits"], r["bad_ids"]) == (35, 2, 2) and r["new_marked_flows"] == 2
    empty = np.zeros(0, abi.FlowMarkRec)
    r = both_update(desc, lens, ids, None, 1, empty, np.zeros(0, mr.MARK_REC), batch_ts=1)   # flow_cap 0, a null table
    assert r == {"n": 70, "hit_packets": 70, "marked_packets": 0, "unkeyed_hits": 4, "bad_ids": 66, "new_marked_flows": 0, "reserved": [0, 0]}
    out, r = abi.flow_mark_select_host(ids, empty, 1)
    assert not out.any() and r == {"n": 70, "n_marked": 0, "n_out": 0, "bad_ids": 66, "reserved": [0, 0, 0, 0]}
    r = abi.flow_mark_update_host(desc[:0], ids[:0], None, 1, got)   # n == 0
    assert r["n"] == 0 and r["hit_packets"] == 0
    out, r = abi.flow_mark_select_host(ids[:0], got, 1)
    assert len(out) == 0 and r == {"n": 0, "n_marked": 0, "n_out": 0, "bad_ids": 0, "reserved": [0, 0, 0, 0]}


@pytest.mark.parametrize("name", GOLDENS)
def test_select_with_every_op_with_and_without_all_bits(name):
    desc, lens, ids, nflows = source(name, ftr.BIDIRECTIONAL)
    n = len(desc)
    table = np.zeros(nflows, mr.MARK_REC)
    mr.update(table, ids, lens, select_words("random", n, 3), 0x1, 5)
    mr.update(table, ids, lens, select_words("random", n, 4), 0x10, 6)
    assert len(set(table["marks"].tolist())) == 4   # 0, 1, 0x10 and 0x11 all occur
    ids = ids.copy()
    ids[5], ids[n - 1] = nflows + 3, 0xFFFFFFFC    # two bad ids
    host = table.view(abi.FlowMarkRec)
    seen = set()
    for op in OPS:
        for flags in (0, mr.ALL_BITS):
            for mask in (0x1, 0x11, 0x100):
                base = select_words("random", n, 9 + op)   # garbage above n
                want, wres = mr.select(table, ids, mask, op, flags, base)
                out, res = abi.flow_mark_select_host(ids, host, mask, op, flags, base=None if op == mr.SET and not flags else base)   # SET takes no base, or ignores one
                assert res == wres and (out == want).all(), (op, flags, mask)
                assert res["bad_ids"] == 2
                if n % 64:
                    assert int(out[-1]) >> (n % 64) == 0
                inplace = base.copy()
                out2, res2 = abi.flow_mark_select_host(ids, host, mask, op, flags, base=inplace, out=inplace)   # base == out
                assert out2 is inplace and res2 == wres and (inplace == want).all()
                seen.add((op, flags, res["n_marked"], res["n_out"]))
    marked = {(op, flags): sorted(m for o, f, m, _ in seen if (o, f) == (op, flags)) for op in OPS for flags in (0, 1)}
    assert all(len(v) >= 2 and v[0] == 0 for v in marked.values())   # mask 0x100 matches nothing; the others differ
    assert marked[(mr.SET, 0)][-1] > marked[(mr.SET, 1)][-1] > 0     # any bit of 0x11 against both


def test_sessions_of_the_goldens_named_in_the_issue():
    """The counts the issue gives: the packets that belong to a flow with a passing packet, against the
    packets that pass, from the goldens' reference verdicts. The tool's test builds on the same numbers."""
    for name, fset, npk, npass, nsess in (("http", "payload_re_11", 3000, 2476, 2531), ("edge", "mixed", 319, 100, 106)):
        g, _ = load_golden(name)
        code = g["code__" + fset]
        n = len(code)
        keys = fr.key_of_rec(g["rec"], False)
        lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
        ids = ftr.expected(*keys, lens)["flow_id"]
        cap = int(ids[ids < 0xFFFFFFF0].max()) + 1
        hit = fr.pack_bits(code == 0)
        got, want = np.zeros(cap, abi.FlowMarkRec), np.zeros(cap, mr.MARK_REC)
        both_update(g["desc"], lens, ids, hit, 1, got, want, batch_ts=1)
        out, res = abi.flow_mark_select_host(ids, got, 1, mr.OR, base=hit.copy())
        assert (n, int((code == 0).sum()), res["n_out"]) == (npk, npass, nsess)
        assert (out == mr.select(want, ids, 1, mr.OR, 0, hit)[0]).all()
        inv, ires = abi.flow_mark_select_host(ids, got, 1, mr.ANDNOT, base=~hit)
        assert ires["n_out"] == n - nsess and not (fr.select_bits(inv, n) & fr.select_bits(out, n)).any()


def test_a_tracker_numbers_the_flows_across_batches():
    """Hits in a later batch mark the flows of an earlier one: flow numbers from flowtrack_ref's tracker."""
    g, _ = load_golden("http")
    keys = fr.key_of_rec(g["rec"], False)
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    n, cap = len(lens), 4096
    ref = fkr.Tracker(cap, ftr.BIDIRECTIONAL)
    got, want = np.zeros(cap, abi.FlowMarkRec), np.zeros(cap, mr.MARK_REC)
    code = g["code__payload_re_11"]
    all_ids = []
    for lo in range(0, n, 256):
        hi = min(n, lo + 256)
        ids = ref.update(keys[0][lo:hi], keys[1][lo:hi], keys[2][lo:hi], lens[lo:hi], None, None, lo)["flow_id"]
        both_update(g["desc"][lo:hi], lens[lo:hi], ids, fr.pack_bits(code[lo:hi] == 0), 1, got, want, batch_ts=lo)
        all_ids.append(ids)
    ids = np.concatenate(all_ids)
    out, res = abi.flow_mark_select_host(ids, got, 1, mr.OR, base=fr.pack_bits(code == 0))
    assert (out == mr.select(want, ids, 1, mr.OR, 0, fr.pack_bits(code == 0))[0]).all()
    assert res["n_out"] > int((code == 0).sum())   # session packets that did not pass themselves


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is
    reported by its own reason."""
    L = abi.lib()
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 16)()
    res = (ctypes.c_uint64 * 4)()
    tsv = (ctypes.c_uint64 * 4)()
    words = (ctypes.c_uint64 * 2)()
    ip, sp, rp, tp, wp = (ctypes.addressof(x) for x in (ids, table, res, tsv, words))

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    ok_upd = abi.FlowMarkUpdate(1, 0, tp, 0)

    def update(word, frames, flow_id=ip, hit=wp, upd=ok_upd, tab=sp, cap=4, result=rp):
        said(L.bt_flow_mark_update_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, hit,
                                          ctypes.byref(upd) if upd is not None else None, tab, cap, result, None), word)

    update("bt_flow_mark_update_device: null context", good())
    update("null context", good(), hit=None, upd=abi.FlowMarkUpdate(0x80000000, 0, None, 5))
    update("null frames", None)
    update("null flow_id", good(), flow_id=None)
    update("null upd", good(), upd=None)
    update("null mark_table", good(), tab=None)
    update("null result", good(), result=None)
    update("mark is 0", good(), upd=abi.FlowMarkUpdate(0, 0, tp, 0))
    update("reserved is not 0", good(), upd=abi.FlowMarkUpdate(1, 1, tp, 0))
    update("mark_table is not 8-byte aligned", good(), tab=sp + 4)
    update("flow_id is not 4-byte aligned", good(), flow_id=ip + 1)
    update("hit is not 8-byte aligned", good(), hit=wp + 4)
    update("ts is not 8-byte aligned", good(), upd=abi.FlowMarkUpdate(1, 0, tp + 4, 0))
    update("result is not 8-byte aligned", good(), result=rp + 4)
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
    update("null context", f, flow_id=None, tab=None, cap=0)   # an empty batch needs no flow_id, flow_cap 0 no table

    def host(word, d=ctypes.addressof(desc), flow_id=ip, hit=wp, upd=ok_upd, tab=sp, cap=4, result=rp):
        said(L.bt_flow_mark_update_host(d, 2, flow_id, hit, ctypes.byref(upd) if upd is not None else None, tab, cap, result), word)

    host("bt_flow_mark_update_host: null desc", d=None)
    host("null flow_id", flow_id=None)
    host("null upd", upd=None)
    host("null mark_table", tab=None)
    host("null result", result=None)
    host("mark is 0", upd=abi.FlowMarkUpdate(0, 0, None, 0))
    host("reserved is not 0", upd=abi.FlowMarkUpdate(1, 9, None, 0))
    host("mark_table is not 8-byte aligned", tab=sp + 4)
    host("ts is not 8-byte aligned", upd=abi.FlowMarkUpdate(1, 0, tp + 1, 0))
    host("result is not 8-byte aligned", result=rp + 4)

    def opts(mask=1, flags=0, op=abi.FLOW_MARK_SET, reserved=0):
        return abi.FlowMarkSelectOpts(mask, flags, op, reserved)

    for fn, name in ((lambda *a: L.bt_flow_mark_select_device(None, *a, None), "bt_flow_mark_select_device"),
                     (L.bt_flow_mark_select_host, "bt_flow_mark_select_host")):
        def sel(word, o=opts(), flow_id=ip, n=2, tab=sp, cap=4, base=None, out=wp, result=rp):
            said(fn(flow_id, n, tab, cap, ctypes.byref(o) if o is not None else None, base, out, result), word)

        sel(name + ": null opts", o=None)
        sel("mask is 0", o=opts(mask=0))
        sel("unknown flag", o=opts(flags=2))
        sel("unknown op", o=opts(op=4))
        sel("reserved is not 0", o=opts(reserved=1))
        sel("null flow_id", flow_id=None)
        sel("null out_select", out=None)
        sel("null mark_table", tab=None)
        sel("null result", result=None)
        sel("flow_id is not 4-byte aligned", flow_id=ip + 2)
        sel("mark_table is not 8-byte aligned", tab=sp + 4)
        sel("base is not 8-byte aligned", base=wp + 4)
        sel("out_select is not 8-byte aligned", out=wp + 4)
        sel("result is not 8-byte aligned", result=rp + 4)
        for op in (abi.FLOW_MARK_AND, abi.FLOW_MARK_OR, abi.FLOW_MARK_ANDNOT):
            sel("this op needs base", o=opts(op=op))
    said(L.bt_flow_mark_select_device(None, ip, 2, sp, 4, ctypes.byref(opts(op=abi.FLOW_MARK_OR)), wp, wp, rp, None), "null context")
    said(L.bt_flow_mark_select_device(None, None, 0, None, 0, ctypes.byref(opts()), None, None, rp, None), "null context")
    assert bytes(table) == bytes(128) and bytes(res) == bytes(32) and bytes(words) == bytes(16)


def test_flowmark_host_check_builds_and_passes(tmp_path):
    """tools/flowmark_host_check.cpp: the argument checks and the two host forms against a naive loop over a
    std::map under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowmark_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flowmark_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
