"""GPU: the per-flow mark side table (bt_flow_mark_update_device, beatrice_amd/csrc/bt_flowmark.hip) and
the selection built from it (bt_flow_mark_select_device). Expected values come from the restatement in
flowmark_ref.py (flow numbers through flowtab_ref / flowtrack_ref, lengths from the descriptors),
never from the code under test; the host forms must agree bit for bit. The table, the words and the
results sit in poisoned buffers between two 256-byte guards and are compared whole; every call is
made twice and the two runs must be byte-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowmark_ref as mr  # noqa: E402
import flowstat_ref as sr  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import FORMATS, POISON, SIZES, Guarded, Source, golden_keys, select_words  # noqa: E402

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
REC = 32
BIG = 3 * 16384 + 17


def stamps(n, seed):
    """Per-packet timestamps that are not in order."""
    return np.uint64(1000) + np.random.default_rng(seed).integers(0, 5000, n).astype(np.uint64)


def upload(ctx, arr):
    d = ctx.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        d.upload(arr)
    return d


def mark_call(ctx, batch, d_ids, hit, mark, cap, want_table, want_res, ts=None, batch_ts=0, start=None, stream=None, where=""):
    """One bt_flow_mark_update_device into a guarded table (zero, or `start`) and a guarded result,
    twice: both runs equal `want` whole and each other. Returns the table's bytes."""
    outs = []
    d_ts = upload(ctx, np.asarray(ts, np.uint64)) if ts is not None else None
    d_hit = upload(ctx, hit) if hit is not None else None
    try:
        for _ in range(2):
            tab, res = Guarded(ctx, REC * cap), Guarded(ctx, 32)
            try:
                if cap:
                    if start is None:
                        abi._check(abi.lib().bt_memset_d(ctx.h, tab.ptr, 0, REC * cap))
                    else:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, start.ctypes.data, REC * cap))
                ctx.synchronize()
                ctx.flow_mark_update(batch, d_ids, d_hit, mark, tab.ptr if cap else None, cap, res.ptr, ts=d_ts, batch_ts=batch_ts, stream=stream)
                if stream is not None:
                    ctx.stream_synchronize(stream)
                ctx.synchronize()
                got = abi.FlowMarkResult.from_bytes(res.read()).as_dict()
                assert got == want_res, f"{where}: result {got} != {want_res}"
                table = tab.read()   # its guards: nothing is written outside mark_table[0 .. flow_cap)
                bad = np.nonzero(table.view(np.uint32) != want_table.view(np.uint32).reshape(-1))[0]
                assert len(bad) == 0, f"{where}: mark table differs at words {bad[:8]} (record {bad[:8] // 8}, word {bad[:8] % 8})"
                outs.append(table.tobytes())
            finally:
                tab.free()
                res.free()
    finally:
        for d in (d_ts, d_hit):
            if d is not None:
                d.free()
    assert outs[0] == outs[1]
    return outs[0]


def select_call(ctx, d_ids, n, table, mask, op, flags, base, in_place=False, stream=None, where=""):
    """One bt_flow_mark_select_device over `table` (host MARK_REC rows, uploaded) into guarded words and a
    guarded result, twice; both equal the restatement and the host form. Returns (words, result)."""
    cap, nw = len(table), (n + 63) // 64
    ids = None
    want, want_res = None, None
    d_tab = upload(ctx, table.view(np.uint8).reshape(-1))
    outs = []
    try:
        ids = d_ids.download(np.zeros(max(n, 1), np.uint32))[:n] if n else np.zeros(0, np.uint32)
        want, want_res = mr.select(table, ids, mask, op, flags, base)
        for _ in range(2):
            out, res = Guarded(ctx, 8 * nw), Guarded(ctx, 32)
            d_base = None
            try:
                if base is not None and nw:
                    if in_place:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, out.ptr, base.ctypes.data, 8 * nw))
                    else:
                        d_base = upload(ctx, base)
                ctx.synchronize()
                ctx.flow_mark_select(d_ids, n, d_tab if cap else None, cap, mask, out.ptr if nw else None, res.ptr, op=op, flags=flags,
                                     base=(out.ptr if in_place else d_base) if base is not None and nw else None, stream=stream)
                if stream is not None:
                    ctx.stream_synchronize(stream)
                ctx.synchronize()
                got = abi.FlowMarkSelectResult.from_bytes(res.read()).as_dict()
                assert got == want_res, f"{where}: result {got} != {want_res}"
                words = out.read(np.uint64)
                bad = np.nonzero(words != want)[0]
                assert len(bad) == 0, f"{where}: words differ at {bad[:8]}: {words[bad[:8]]} != {want[bad[:8]]}"
                outs.append(words.tobytes())
            finally:
                out.free()
                res.free()
                if d_base is not None:
                    d_base.free()
        if n:
            hout, hres = abi.flow_mark_select_host(ids, table.view(abi.FlowMarkRec), mask, op, flags, base=base)
            assert hres == want_res and hout.tobytes() == outs[0], f"{where}: the host form"
    finally:
        d_tab.free()
    assert outs[0] == outs[1]
    return want, want_res


def golden_case(ctx, name, n, fmt, kind, per_packet_ts, where, mark=0x4, stream=None):
    """A golden repeated to n packets with flowtab_ref's flow ids: an update into a zero table, then
    selections over the table it leaves."""
    src = Source(ctx, name, n, fmt)
    want_all = src.want(0)
    ids, nflows = want_all["flow_id"], want_all["result"]["n_flows"]
    cap = nflows + 2
    d_ids = upload(ctx, ids)
    try:
        hit = select_words(kind, n)
        ts = stamps(n, n) if per_packet_ts and n else None
        want = np.zeros(cap, mr.MARK_REC)
        want_res = mr.update(want, ids, src.lens, hit, mark, 4242 if ts is None else ts)
        got = mark_call(ctx, src.batch, d_ids, hit, mark, cap, want, want_res, ts=ts, batch_ts=4242, stream=stream, where=where)
        if fmt == "packed" and n:   # the host form, bit for bit
            host = np.zeros(cap, abi.FlowMarkRec)
            assert abi.flow_mark_update_host(src.desc, ids, hit, mark, host, ts=ts, batch_ts=4242) == want_res
            assert host.tobytes() == got
        base = select_words("random", n, seed=5)
        select_call(ctx, d_ids, n, want, mark, mr.OR, 0, base, stream=stream, where=where + " OR")
        select_call(ctx, d_ids, n, want, mark | 0x100, mr.SET, mr.ALL_BITS if n % 2 else 0, None, stream=stream, where=where + " SET")
        return want_res
    finally:
        src.free()
        d_ids.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    """c3 cycled to every size, so that flows span waves, blocks and chunks; the format and the hit words
    rotate (the lengths differ by format); per-packet stamps on the odd cases."""
    si = SIZES.index(n)
    res = golden_case(gpu_ctx, "c3", n, FORMATS[si % 3], ("random", "null", "ones")[si % 3], si % 2 == 1, f"c3 n={n}")
    assert res["n"] == n and (n == 0 or res["marked_packets"] > 0) and res["bad_ids"] == 0


@pytest.mark.parametrize("name,fmt", [("edge", "xdp"), ("http", "stride"), ("http", "packed")])
def test_sources_with_packets_that_have_no_key(gpu_ctx, name, fmt):
    """edge and http repeated two and a half times, on a stream of its own: hits without a key are counted, not marked."""
    g, _ = load_golden(name)
    st = gpu_ctx.stream_create()
    try:
        res = golden_case(gpu_ctx, name, len(g["desc"]) * 5 // 2, fmt, "random", fmt != "xdp", f"{name} {fmt}", mark=0x80000001, stream=st)
        assert res["unkeyed_hits"] > 0 and res["marked_packets"] > res["new_marked_flows"] > 0
    finally:
        gpu_ctx.stream_destroy(st)


def crafted(ctx, lens, ids, hit, mark, cap, where, ts=None, batch_ts=0, start=None, fmt="packed"):
    """Descriptors with the caller's lengths and flow ids (no frame byte is read): the restatement and the host form."""
    n = len(ids)
    lens, ids = np.asarray(lens, np.uint64), np.asarray(ids, np.uint32)
    desc = ((np.arange(n, dtype=np.uint64) % np.uint64(64)) * np.uint64(64)) | (lens << np.uint64(48))
    src = Source(ctx, "edge", n, fmt, data=np.zeros(4096, np.uint8), desc=desc)
    d_ids = upload(ctx, ids)
    try:
        want = np.zeros(cap, mr.MARK_REC) if start is None else start.copy()
        want_res = mr.update(want, ids, lens.astype(np.int64), hit, mark, batch_ts if ts is None else ts)
        got = mark_call(ctx, src.batch, d_ids, hit, mark, cap, want, want_res, ts=ts, batch_ts=batch_ts, start=start, where=where)
        host = np.zeros(cap, abi.FlowMarkRec) if start is None else start.copy().view(abi.FlowMarkRec)
        assert abi.flow_mark_update_host(desc, ids, hit, mark, host, ts=ts, batch_ts=batch_ts) == want_res, where
        assert host.tobytes() == got, f"{where}: the host form"
        return want, want_res
    finally:
        src.free()
        d_ids.free()


@pytest.mark.parametrize("hit_kind,fmt", [("null", "packed"), ("ones", "xdp")])
def test_every_packet_a_hit_of_one_flow(gpu_ctx, hit_kind, fmt):
    """3 * 16384 + 17 packets on one record: the sums wait in the waves and are exact; the earliest and the
    latest stamp sit at the last lane of a tile and at the first packet of the last block. The record starts
    close to the wrap of hit_packets."""
    n = BIG
    lens = 60 + (np.arange(n) * 7) % 1400
    lens[[0, 63, 16384, n - 1]] = 65535
    ts = np.uint64(100000) + (np.arange(n, dtype=np.uint64) * np.uint64(7919)) % np.uint64(50000)
    ts[63], ts[3 * 16384] = 7, U64_MAX - 1
    start = np.zeros(2, mr.MARK_REC)
    start["marks"], start["hit_packets"], start["hit_bytes"] = 0x10, 0xFFFFFFF0, U64_MAX - 1000
    start["first_hit_ts_c"][1], start["last_hit_ts"][1] = 5, 6
    want, res = crafted(gpu_ctx, lens, np.zeros(n, np.uint32), select_words(hit_kind, n), 0x3, 2, f"one flow {hit_kind}", ts=ts, start=start, fmt=fmt)
    assert res == {"n": n, "hit_packets": n, "marked_packets": n, "unkeyed_hits": 0, "bad_ids": 0, "new_marked_flows": 1, "reserved": [0, 0]}
    d = abi.decode_flow_mark(want[0])
    assert d == {"marks": 0x13, "hit_packets": (0xFFFFFFF0 + n) % (1 << 32), "hit_bytes": (U64_MAX - 1000 + int(lens.sum())) % (1 << 64),
                 "first_hit_ts": 7, "last_hit_ts": U64_MAX - 1}
    assert want[1].tobytes() == start[1].tobytes()


def test_every_packet_a_hit_of_its_own_flow(gpu_ctx):
    """c1: 10,000 packets, 10,000 flows, every lane alone in its tile."""
    res = golden_case(gpu_ctx, "c1", 10000, "packed", "null", True, "c1")
    assert res["marked_packets"] == res["new_marked_flows"] == 10000


def test_64_flows_in_one_tile_slots_shared_and_pairs(gpu_ctx):
    """Flow numbers 256 apart share a byte of the wave's table of lone lanes; then a second lane of flow 0 at
    the tile's end; two flows interleaved over three tiles, so that the waiting sums are flushed."""
    lens = 54 + np.arange(64) % 11
    ids = np.concatenate([np.arange(32, dtype=np.uint32), 256 + np.arange(32, dtype=np.uint32)])
    want, res = crafted(gpu_ctx, lens, ids, None, 1, 288, "flows 256 apart", ts=stamps(64, 3))
    assert res["new_marked_flows"] == 64 and int((want["hit_packets"] == 1).sum()) == 64
    ids[63] = 0
    want, res = crafted(gpu_ctx, lens, ids, None, 1, 288, "flows 256 apart and a pair", ts=stamps(64, 4))
    assert res["new_marked_flows"] == 63 and int(want["hit_packets"][0]) == 2 and int(want["hit_bytes"][0]) == 54 + 54 + 63 % 11
    ids = np.arange(130, dtype=np.uint32) % 2
    want, res = crafted(gpu_ctx, 60 + np.arange(130), ids, select_words("random", 130, 8), 2, 2, "two flows", batch_ts=3)
    assert res["new_marked_flows"] == 2 and int(want["hit_packets"].sum()) == res["hit_packets"] > 40
    # sentinels are unkeyed hits; 0xFFFFFFFC and ids at or past flow_cap are bad ids; flow_cap 0 takes a null table
    ids = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 0xFFFFFFFC, 5, 6, 4] + [4] * 54, np.uint32)
    _, res = crafted(gpu_ctx, lens, ids, None, 1, 5, "sentinels and bad ids", batch_ts=9)
    assert (res["unkeyed_hits"], res["bad_ids"], res["marked_packets"], res["new_marked_flows"]) == (4, 3, 57, 3)
    _, res = crafted(gpu_ctx, lens, ids, fr.pack_bits(np.arange(64) % 2 == 1), 1, 5, "ids of packets that are no hit are not looked at", batch_ts=9)
    assert (res["hit_packets"], res["unkeyed_hits"], res["bad_ids"]) == (32, 2, 1)
    _, res = crafted(gpu_ctx, lens, np.arange(64, dtype=np.uint32), None, 1, 0, "flow_cap 0")
    assert res == {"n": 64, "hit_packets": 64, "marked_packets": 0, "unkeyed_hits": 0, "bad_ids": 64, "new_marked_flows": 0, "reserved": [0, 0]}


@pytest.mark.parametrize("which", ["first", "last", "bit 63 of a middle word"])
def test_one_hit_bit_in_the_whole_batch(gpu_ctx, which):
    n = BIG
    i = {"first": 0, "last": n - 1, "bit 63 of a middle word": 64 * 300 + 63}[which]
    bits = np.zeros(n, bool)
    bits[i] = True
    hit = fr.pack_bits(bits)
    if which != "last":
        hit[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # garbage at or above n
    ids = (np.arange(n, dtype=np.uint32) * 7) % 1000
    want, res = crafted(gpu_ctx, 60 + np.arange(n) % 1000, ids, hit, 0x8, 1000, which, ts=stamps(n, 6))
    assert res == {"n": n, "hit_packets": 1, "marked_packets": 1, "unkeyed_hits": 0, "bad_ids": 0, "new_marked_flows": 1, "reserved": [0, 0]}
    assert int((want["marks"] != 0).sum()) == 1 and int(want["hit_bytes"][ids[i]]) == 60 + i % 1000


def test_hit_words_all_zero_leave_the_table_untouched(gpu_ctx):
    n = 16385
    start = np.frombuffer(np.random.default_rng(1).bytes(REC * 40), mr.MARK_REC).copy()
    want, res = crafted(gpu_ctx, np.full(n, 100), np.arange(n, dtype=np.uint32) % 40, select_words("zeros", n), 1, 40, "no hits", start=start)
    assert want.tobytes() == start.tobytes() and res == {"n": n, "hit_packets": 0, "marked_packets": 0, "unkeyed_hits": 0, "bad_ids": 0,
                                                         "new_marked_flows": 0, "reserved": [0, 0]}


def test_a_table_that_already_holds_the_bit(gpu_ctx):
    """No record changes in marks and no flow is new; a mark of two bits, one of them held, makes every hit flow new."""
    n, cap = 16385, 300
    start = np.zeros(cap, mr.MARK_REC)
    start["marks"] = 0x44
    start["last_hit_ts"] = 10 ** 9   # later than every stamp: no atomic for it either
    ids = (np.arange(n, dtype=np.uint32) * 7) % 299
    want, res = crafted(gpu_ctx, np.full(n, 64), ids, None, 0x4, cap, "the bit is there", ts=stamps(n, 7), start=start)
    assert res["new_marked_flows"] == 0 and (want["marks"] == 0x44).all() and (want["last_hit_ts"] == 10 ** 9).all()
    assert int(want["hit_packets"].sum()) == n and not want["hit_packets"][299]
    want, res = crafted(gpu_ctx, np.full(n, 64), ids, None, 0x6, cap, "one bit of two is there", batch_ts=5, start=start)
    assert res["new_marked_flows"] == 299 and (want["marks"][:299] == 0x46).all() and want["marks"][299] == 0x44


@pytest.mark.parametrize("n", [1, 63, 65, 16385, BIG])
def test_select_every_op_with_a_garbage_base_and_in_place(gpu_ctx, n):
    """n % 64 != 0: the bits at or above n come out 0 whatever base holds there; base == out_select in place."""
    cap = 500
    table = np.zeros(cap, mr.MARK_REC)
    table["marks"] = np.random.default_rng(n).integers(0, 4, cap).astype(np.uint32) * np.uint32(0x11) & np.uint32(0x21)   # 0, 0x1, 0x20, 0x21
    ids = np.random.default_rng(n + 1).integers(0, cap, n).astype(np.uint32)
    ids[::17] = 0xFFFFFFFE
    ids[n // 2] = cap   # a bad id
    d_ids = upload(gpu_ctx, ids)
    try:
        k = 0
        for op in (mr.SET, mr.AND, mr.OR, mr.ANDNOT):
            for flags in (0, mr.ALL_BITS):
                base = select_words("random" if op != mr.ANDNOT else "ones", n, seed=op)
                assert int(base[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1
                want, res = select_call(gpu_ctx, d_ids, n, table, 0x21, op, flags, base, in_place=(k % 2 == 1), where=f"n={n} op={op} flags={flags}")
                assert int(want[-1]) >> (n % 64) == 0 and res["bad_ids"] == 1 and res["n"] == n
                k += 1
        _, res = select_call(gpu_ctx, d_ids, n, table[:0], 1, mr.SET, 0, None, where="flow_cap 0")
        assert res["n_marked"] == 0 and res["bad_ids"] == int((ids != 0xFFFFFFFE).sum())
    finally:
        d_ids.free()


def test_behind_the_tracker_on_a_callers_stream_and_through_an_expire(gpu_ctx):
    """Two batches of http: tracker update, mark update (the hits: the reference's verdicts) and select,
    enqueued on a caller's stream with no host synchronisation between; then an expire and the generic side
    move with rec_bytes 32: the mark table equals the restatement's move, expired_side[k] belongs to expired[k]."""
    ctx = gpu_ctx
    g, _ = load_golden("http")
    code = g["code__payload_re_11"]
    keys = golden_keys("http", False)
    flags, cap, xcap = ftr.BIDIRECTIONAL, 2400, 2400
    cuts = [(0, 1700), (1700, 3000)]
    lay = abi.flow_track_layout(cap)
    need, xneed, mneed = abi.flow_track_scratch_bytes(1700), abi.flow_track_expire_scratch_bytes(cap), abi.flow_track_side_move_scratch_bytes(cap, REC)
    ref, want = fkr.Tracker(cap, flags), np.zeros(cap, mr.MARK_REC)
    runs, expect = [], []
    for _ in range(2):
        state, marks = Guarded(ctx, lay["total"]), Guarded(ctx, REC * cap)
        exp, gone, remap, xres = Guarded(ctx, 104 * xcap), Guarded(ctx, REC * xcap), Guarded(ctx, 4 * cap), Guarded(ctx, 32)
        xscratch, mscratch = Guarded(ctx, xneed), Guarded(ctx, mneed)
        bufs, per = [state, marks, exp, gone, remap, xres, xscratch, mscratch], []
        st = ctx.stream_create()
        try:
            abi._check(abi.lib().bt_memset_d(ctx.h, marks.ptr, 0, REC * cap))
            ctx.synchronize()
            ctx.flow_track_init(state.ptr, lay["total"], cap, flags, stream=st)
            for b, (lo, hi) in enumerate(cuts):
                n = hi - lo
                src = Source(ctx, "http", n, "packed", desc=g["desc"][lo:hi])
                hit = fr.pack_bits(code[lo:hi] == 0)
                ids, res, scratch, mres, sel, sres = (Guarded(ctx, 4 * n), Guarded(ctx, 64), Guarded(ctx, need), Guarded(ctx, 32),
                                                      Guarded(ctx, 8 * ((n + 63) // 64)), Guarded(ctx, 32))
                d_hit = upload(ctx, hit)
                bufs += [src, ids, res, scratch, mres, sel, sres, d_hit]
                per.append((lo, hi, hit, ids, mres, sel, sres))
                ctx.synchronize()   # the uploads; nothing between the three calls below
                ctx.flow_track_update(state.ptr, src.batch, scratch.ptr, need, res.ptr, batch_ts=100 * b, flow_id=ids.ptr, stream=st)
                ctx.flow_mark_update(src.batch, ids.ptr, d_hit, 1, marks.ptr, cap, mres.ptr, batch_ts=100 * b, stream=st)
                ctx.flow_mark_select(ids.ptr, n, marks.ptr, cap, 1, sel.ptr, sres.ptr, op=mr.OR, base=d_hit, stream=st)
            ctx.flow_track_expire(state.ptr, 100, 50, xscratch.ptr, xneed, xres.ptr, expired=exp.ptr, expired_cap=xcap, remap=remap.ptr, stream=st)
            ctx.flow_track_side_move(marks.ptr, REC, cap, remap.ptr, xres.ptr, mscratch.ptr, mneed, expired_side=gone.ptr, expired_cap=xcap, stream=st)
            ctx.stream_synchronize(st)
            ctx.synchronize()
            first = not runs
            for b, (lo, hi, hit, ids, mres, sel, sres) in enumerate(per):
                got_ids = ids.read(np.uint32)
                if first:
                    lens = (g["desc"][lo:hi] >> np.uint64(48)).astype(np.int64)
                    wid = ref.update(keys[0][lo:hi], keys[1][lo:hi], keys[2][lo:hi], lens, None, None, 100 * b)["flow_id"]
                    wres = mr.update(want, wid, lens, hit, 1, 100 * b)
                    expect.append((wid, wres) + mr.select(want, wid, 1, mr.OR, 0, hit))
                wid, wres, wsel, wsres = expect[b]
                assert (got_ids == wid).all(), f"batch {b}: flow ids"
                assert abi.FlowMarkResult.from_bytes(mres.read()).as_dict() == wres, f"batch {b}: mark result"
                assert abi.FlowMarkSelectResult.from_bytes(sres.read()).as_dict() == wsres and (sel.read(np.uint64) == wsel).all(), f"batch {b}: select"
                assert wsres["n_out"] > int(fr.select_bits(hit, hi - lo).sum())
            if first:
                xwant = ref.expire(100, 50, xcap)
                want_gone = sr.side_move(want, xwant["remap"], xwant["result"], xcap)
            x = abi.FlowTrackExpireResult.from_bytes(xres.read()).as_dict()
            assert x == xwant["result"] and x["n_expired"] > 0 and x["n_flows"] > 0
            ne = x["n_expired"]
            table, g_side, g_exp = marks.read(), gone.read(), exp.read()
            assert table.tobytes() == want.tobytes(), "the mark table behind the move"
            assert g_side[:REC * ne].tobytes() == want_gone.tobytes() and (g_side[REC * ne:] == POISON).all()
            assert want_gone["marks"].any() and not want_gone["marks"].all()
            # expired_side[k] belongs to expired[k]: a marked flow's hits are no more than the flow's packets, and its stamps lie within the flow's
            recs = g_exp[:104 * ne].view(abi.FlowTrackRec)
            side = g_side[:REC * ne].view(abi.FlowMarkRec)
            assert (side["hit_packets"] <= recs["packets"].sum(axis=1)).all() and (side["hit_bytes"] <= recs["bytes"].sum(axis=1)).all()
            hitrows = side["marks"] != 0
            assert (side["last_hit_ts"][hitrows] <= recs["last_ts"][hitrows]).all()
            mscratch.read()
            runs.append(table.tobytes() + g_side.tobytes())
        finally:
            abi.Context.flow_track_forget(state.ptr)
            ctx.stream_destroy(st)
            for x_ in bufs:
                x_.free()
    assert runs[0] == runs[1]
