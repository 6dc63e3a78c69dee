"""GPU: TCP segments classified per flow and direction against the sequence space
(bt_flow_tcpseq_device, beatrice_amd/csrc/bt_flowtcpseq.hip). The kernels take flow_id directly, so the ids
are crafted. Every device call is compared bit for bit with the host form (classes, offsets, selection
words, table, result) and with the restatement in flowtcpseq_ref.py (Python integers, a dict per
direction), and where the case generator knows it, with the classes that follow from the true 64-bit
offsets. The outputs, the table, the result and the scratch sit in poisoned buffers between two 256-byte
guards; the scratch is filled with 0xA5 first; every call is made twice from the same starting table and
the two runs must be byte-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowstat_ref as str_  # noqa: E402
import flowtcpseq_cases as tc  # noqa: E402
import flowtcpseq_ref as tr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowstream import words_of  # noqa: E402
from test_gpu_flowstream import Frames, upload  # noqa: E402
from test_gpu_flowtab import FORMATS, Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

BIDIR = 2
UNIT, CHUNK = 2048, 16384   # kFsUnit, kFsChunk
REC = 128
OUTS = ("cls", "off", "out_select")


def device_once(ctx, batch, n, d_ids, sel, flags, cap, tab_ptr, outs=OUTS, in_place=False, stream=None):
    """One bt_flow_tcpseq_device into guarded outputs, a guarded result and a guarded scratch full of 0xA5.
    Returns (cls, off, out_select, each None where not asked for; the result dict)."""
    nw = (n + 63) // 64
    need = abi.flow_tcpseq_scratch_bytes(n, cap)
    cls = Guarded(ctx, n) if "cls" in outs else None
    off = Guarded(ctx, 8 * n) if "off" in outs else None
    osel = Guarded(ctx, 8 * nw) if "out_select" in outs or in_place else None
    res, scratch = Guarded(ctx, 64), Guarded(ctx, need)
    d_sel = None
    try:
        abi._check(abi.lib().bt_memset_d(ctx.h, scratch.ptr, 0xA5, need))
        if sel is not None and nw:
            if in_place:
                abi._check(abi.lib().bt_memcpy_h2d(ctx.h, osel.ptr, sel.ctypes.data, 8 * nw))
            else:
                d_sel = upload(ctx, sel)
        ctx.synchronize()
        sel_ptr = None if sel is None or not nw else osel.ptr if in_place else d_sel
        ctx.flow_tcpseq(batch, d_ids, sel_ptr, flags, tab_ptr if cap else None, cap, scratch.ptr if n else None, need, res.ptr,
                        cls=cls.ptr if cls and n else None, off=off.ptr if off and n else None,
                        out_select=osel.ptr if osel and nw else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        scratch.read()   # its guards
        out = abi.FlowTcpseqResult.from_bytes(res.read()).as_dict()
        return (cls.read() if cls else None, off.read(np.int64) if off else None, osel.read(np.uint64) if osel else None, out)
    finally:
        for g in (cls, off, osel, res, scratch, d_sel):
            if g is not None:
                g.free()


def run_case(ctx, batches, cap, flags=BIDIR, fmt="packed", start=None, in_place=False, stream=None, where="", outs=OUTS, truth=True):
    """batches: [(frames, ids, select bits, rows or None)]. Per batch: the restatement, the device call twice from
    the same table, the host form, the generator's truth; the table carries on. Returns (the restatement,
    [(cls, off, out_select)], [result])."""
    model = tr.Space(cap, flags, start)
    table = np.zeros(cap, tr.REC) if start is None else start.copy()
    got, results = [], []
    for k, (frames, ids, bits, rows) in enumerate(batches):
        at = f"{where} batch {k}"
        n, ids = len(frames), np.ascontiguousarray(ids, np.uint32)
        src = Frames(ctx, frames, fmt)
        d_ids = upload(ctx, ids)
        sel = None if all(bits) and not in_place else words_of(bits)
        if sel is not None and n % 64:
            sel[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
        wcls, woff, wsel, want_res = model.batch(src.seen, ids, sel)
        wtab = model.table
        runs = []
        try:
            for _ in range(2):
                tab = Guarded(ctx, REC * cap)
                try:
                    if cap:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, table.ctypes.data, REC * cap))
                    cls, off, osel, res = device_once(ctx, src.batch, n, d_ids, sel, flags, cap, tab.ptr, outs, in_place, stream)
                    after = tab.read()
                finally:
                    tab.free()
                assert res == want_res, f"{at}: result {res} != {want_res}"
                cls = wcls if cls is None else cls   # not asked for: everything else is the same
                off = woff if off is None else off
                osel = wsel if osel is None else osel
                bad = np.nonzero(cls != wcls)[0]
                assert len(bad) == 0, f"{at}: class differs at packets {bad[:8]} (ids {ids[bad[:8]]}): {cls[bad[:8]]} != {wcls[bad[:8]]}"
                bad = np.nonzero(off != woff)[0]
                assert len(bad) == 0, f"{at}: off differs at packets {bad[:8]}: {off[bad[:8]]} != {woff[bad[:8]]}"
                assert (osel == wsel).all(), f"{at}: out_select"
                rows_bad = np.nonzero((after.view(np.uint64).reshape(-1, 16) != wtab.view(np.uint64).reshape(-1, 16)).any(axis=1))[0]
                assert len(rows_bad) == 0, f"{at}: table differs at flows {rows_bad[:8]}: {after.view(tr.REC)[rows_bad[:2]]} != {wtab[rows_bad[:2]]}"
                runs.append((cls.tobytes(), off.tobytes(), osel.tobytes(), after.tobytes()))
            assert runs[0] == runs[1], f"{at}: two runs differ"
            if n:   # the host form, bit for bit
                host = table.copy().view(abi.FlowTcpseqRec)
                hcls, hoff, hsel = np.full(n, 0xEE, np.uint8), np.full(n, 7, np.int64), np.full((n + 63) // 64, 0xDEAD, np.uint64)
                hres = abi.flow_tcpseq_host(src.data, src.desc, ids, sel, flags, host, cls=hcls, off=hoff, out_select=hsel)
                assert hres == want_res and (hcls.tobytes(), hoff.tobytes(), hsel.tobytes(), host.tobytes()) == runs[0], f"{at}: the host form"
            if truth and rows is not None:
                mine = [(int(c), None if int(o) == tr.OFF_NONE else int(o)) for c, o in zip(wcls, woff)]
                assert mine == [(r.want, r.u) for r in rows], f"{at}: the generator's truth"
        finally:
            src.free()
            d_ids.free()
        table = wtab.copy()
        got.append((wcls, woff, wsel))
        results.append(want_res)
    return model, got, results


def test_the_named_cases(gpu_ctx):
    """flowtcpseq_cases.crafted: the wrap mid-stream, SYN and FIN and their retransmits, a loss, the hole filled
    late, an overlap, RST, IP options, a tag, TCP options, padding, IPv6, snapped frames, what does not
    participate, a step of 2^31, sentinels and bad ids; over two batches, with and without directions."""
    rows, cap = tc.crafted()
    _, _, results = run_case(gpu_ctx, tc.batches_of(rows), cap, BIDIR, where="crafted")
    assert results[0]["unkeyed"] + results[1]["unkeyed"] == 4 and results[0]["bad_ids"] + results[1]["bad_ids"] == 2
    run_case(gpu_ctx, tc.batches_of(rows), cap, 0, truth=False, where="crafted, one direction")


def test_the_gap_this_feature_closes(gpu_ctx):
    """HE, LL, LL again, O: the arrival-order stream reads HELLLLO, so the stream matcher misses HELLO; with
    this call's out_select in front of it the retransmit stays out and the last packet is hit."""
    from test_gpu_flowstream import Pattern, device_once as stream_once
    ctx = gpu_ctx
    frames = [tc.tcp(100, payload=b"HE"), tc.tcp(102, payload=b"LL"), tc.tcp(102, payload=b"LL"), tc.tcp(104, payload=b"O")]
    rows = tc.truth([tc.Row(f, 0, True, (0, 0), o, ln) for f, o, ln in zip(frames, (0, 2, 2, 4), (2, 2, 2, 1))])
    _, got, _ = run_case(ctx, [(frames, [0] * 4, [True] * 4, rows)], 1, where="HELLO")
    assert int(got[0][2][0]) == 0b1011
    pat, src, d_ids = Pattern(ctx, "HELLO"), Frames(ctx, frames, "packed"), upload(ctx, np.zeros(4, np.uint32))
    try:
        for sel, want in ((np.array([0b1111], np.uint64), 0), (got[0][2], 0b1000)):
            tab = Guarded(ctx, 32)
            try:
                abi._check(abi.lib().bt_memset_d(ctx.h, tab.ptr, 0, 32))
                hit, _ = stream_once(ctx, pat, src.batch, 4, d_ids, sel, BIDIR, 1, tab.ptr)
                tab.read()
            finally:
                tab.free()
            assert int(hit[0]) == want
    finally:
        for x in (pat, src, d_ids):
            x.free()


def mixed_batch(n, seed, nflows):
    """n packets of random conversations over nflows flows, cut or repeated to n, with sentinels, bad ids and
    unselected packets."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        rows += tc.random_set(seed + len(rows), nflows=nflows, nseg=max(2, min(40, n // (2 * nflows))))
    rows = tc.truth([r.again() for r in rows[:n]])
    frames, ids = [r.frame for r in rows], np.array([r.flow for r in rows], np.uint32)
    if n > 70:
        ids[rng.integers(0, n, 1 + n // 50)] = 0xFFFFFFFE
        ids[rng.integers(0, n, 1 + n // 90)] = nflows + 5
    return frames, ids, [bool(x) for x in rng.integers(0, 6, n)], None


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_at_tile_edges(gpu_ctx, n):
    batches = [mixed_batch(n, n, 3), mixed_batch(n, n + 1, 3)]
    _, _, results = run_case(gpu_ctx, batches, 3, where=f"n={n}")
    assert results[0]["n"] == n and results[1]["n"] == n


def test_a_batch_with_no_tcp_at_all(gpu_ctx):
    frames = [tc.tcp(k, 10, proto=17) for k in range(150)] + [tc.tcp(k, 0) for k in range(50)]
    _, got, results = run_case(gpu_ctx, [(frames, [k % 5 for k in range(200)], [True] * 200, None)], 5, where="m=0")
    assert results[0]["seq_packets"] == 0 and results[0]["selected"] == 200 and not got[0][0].any()


@pytest.mark.parametrize("n,dups", [(UNIT + 1, (UNIT - 1, UNIT)), (UNIT + 1, (1, UNIT // 2)), (CHUNK + 1, (CHUNK - 1, CHUNK, UNIT))])
def test_one_direction_across_a_unit_and_a_chunk(gpu_ctx, n, dups):
    """One (flow, direction) segment of 2,049 and of 16,385 participating packets; a duplicate as the last
    packet of a unit and as the first of the next."""
    rows = tc.truth(tc.one_direction(n, dup_at=dups))
    model, got, results = run_case(gpu_ctx, [([r.frame for r in rows], [0] * n, [True] * n, rows)], 1, where=f"one direction n={n}")
    assert results[0]["old"] == len(dups) and results[0]["in_order"] == n - 1 - len(dups) and results[0]["first"] == 1
    assert int(model.table[0]["d"][0]["hi"]) == 3 * (n - len(dups)) and [int(got[0][0][k]) for k in dups] == [tc.OLD] * len(dups)


@pytest.mark.parametrize("edge", [UNIT, CHUNK])
def test_a_head_exactly_at_a_unit_and_a_chunk_edge(gpu_ctx, edge):
    """Flow 0 has exactly `edge` participating packets, so flow 1's head sits at that sorted position; flow 1
    goes on from a record with a state."""
    a = tc.one_direction(edge, dup_at=(5, edge - 1), flow=0)
    b = tc.one_direction(70, dup_at=(1,), flow=1, isn=0xFFFFFFC0)
    start = np.zeros(2, tr.REC)
    s = start[1]["d"][0]
    s["have"], s["pos"], s["hi"], s["last_seq"], s["seq_packets"] = 1, 5000, 5030, (0xFFFFFFC0 - 3) & tc.M32, 0xFFFFFFFF
    rows = [r for pair in zip(a, b) for r in pair] + a[len(b):]   # interleaved in arrival
    batch = ([r.frame for r in rows], [r.flow for r in rows], [True] * len(rows), None)
    model, got, results = run_case(gpu_ctx, [batch], 2, start=start, where=f"head at {edge}")
    assert results[0]["seq_packets"] == edge + 70 and results[0]["first"] == 1
    first_b = [k for k, r in enumerate(rows) if r.flow == 1][0]
    assert int(got[0][0][first_b]) == tc.OLD and int(got[0][1][first_b]) == 5003   # 3 bytes at 5003 below hi = 5030
    assert int(model.table[1]["d"][0]["seq_packets"]) == 69   # wrapped


def test_round_robin_over_seven_flows_in_both_directions(gpu_ctx):
    """About 3,000 packets, flow by flow in turn: heads fall mid-tile and a step is read across tile and unit edges."""
    conns = [tc.Conn(f, tc.M32 - 30 - f, 1 << 31, sp=44000 + f) for f in range(7)]
    rng = np.random.default_rng(7)
    at = {}
    rows = []
    for k in range(3010):
        f, d = k % 7, (k // 7) % 2
        off = at.get((f, d), 0)
        op = int(rng.integers(0, 8))
        ln = int(rng.integers(1, 30))
        if op == 0 and off:
            rows.append(conns[f].seg(d, off - min(off, 10), ln))    # old or overlapping
        elif op == 1:
            rows.append(conns[f].seg(d, off + 13, ln))             # a loss in front
        else:
            rows.append(conns[f].seg(d, off, ln))
        at[(f, d)] = max(off, rows[-1].off + ln)
    rows = tc.checked(rows)
    _, _, results = run_case(gpu_ctx, [([r.frame for r in rows], [r.flow for r in rows], [True] * len(rows), rows)], 7, where="round robin")
    assert min(results[0][k] for k in ("first", "in_order", "gap", "old", "overlap")) > 0 and results[0]["first"] == 14


def test_state_carried_over_three_calls_with_a_wrap_in_the_middle_one(gpu_ctx):
    c = tc.Conn(0, tc.M32 + 1 - 60, tc.M32 + 1 - 3000)   # direction 1 wraps at its 31st segment
    rows = []
    for b, (lo, hi) in enumerate(((0, 20), (20, 50), (50, 70))):
        for k in range(lo, hi):
            for d in range(2):
                r = c.seg(d, 100 * k, 100)
                r.batch = b
                rows.append(r)
            if k % 9 == 4:
                r = c.seg(0, 100 * k + 50, 100)   # overlaps
                r.batch = b
                rows.append(r)
            if k % 9 == 7:
                r = c.seg(1, 100 * k, 100)        # a retransmit
                r.batch = b
                rows.append(r)
    extra = c.seg(0, 7100, 10)                    # a loss of 100
    extra.batch = 2
    rows = tc.checked(rows + [extra])
    model, _, results = run_case(gpu_ctx, tc.batches_of(rows), 1, where="three calls")
    assert results[1]["first"] == 0 and results[1]["in_order"] >= 50 and int(model.table[0]["d"][0]["hi"]) == 7110
    assert int(model.table[0]["d"][1]["last_seq"]) == (c.isn[1] + 6900) & tc.M32 == 3900   # wrapped


@pytest.mark.parametrize("cap", [1, 257])
def test_flow_caps_of_one_and_two_radix_passes(gpu_ctx, cap):
    """The sort key is flow << 1 | direction: flow_cap 1 sorts in one pass, 257 needs two."""
    frames, ids, bits, _ = mixed_batch(900, cap, min(cap, 6))
    if cap > 1:
        ids[ids < cap] = (ids[ids < cap].astype(np.int64) * 51 % cap).astype(np.uint32)   # 0, 51, .., 255 and 256
        ids[::97] = cap - 1
    _, _, results = run_case(gpu_ctx, [(frames, ids, bits, None), (frames[::-1], ids[::-1], bits[::-1], None)], cap, where=f"cap={cap}")
    assert results[0]["seq_packets"] > 300 and results[1]["old"] > 100


@pytest.mark.parametrize("outs", [(), ("cls",), ("off",), ("out_select",), ("cls", "off")])
def test_each_output_absent_in_turn(gpu_ctx, outs):
    for given in (True, False):
        frames, ids, bits, _ = mixed_batch(UNIT + 70, 5, 5)
        if not given:
            bits = [True] * len(bits)
        _, _, results = run_case(gpu_ctx, [(frames, ids, bits, None)], 5, outs=outs, where=f"outs={outs} select={given}")
        assert results[0]["unkeyed"] > 0 and results[0]["bad_ids"] > 0 and results[0]["old"] > 0


def test_out_select_in_place_of_select(gpu_ctx):
    _, got, results = run_case(gpu_ctx, [mixed_batch(UNIT + 300, 8, 9)], 9, in_place=True, where="in place")
    assert 0 < results[0]["old"] < results[0]["seq_packets"] < results[0]["selected"] < UNIT + 300
    assert sum(bin(int(w)).count("1") for w in got[0][2]) == results[0]["selected"] - results[0]["old"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_descriptor_formats_on_a_stream_of_its_own(gpu_ctx, fmt):
    st = gpu_ctx.stream_create()
    try:
        rows = tc.random_set(17, nflows=5, nseg=30)
        batch = ([r.frame for r in rows], [r.flow for r in rows], [True] * len(rows), rows)
        _, _, results = run_case(gpu_ctx, [batch], 5, fmt=fmt, stream=st, where=fmt)
        assert results[0]["old"] > 3 and results[0]["gap"] > 0
    finally:
        gpu_ctx.stream_destroy(st)


def test_the_table_goes_through_a_device_expire_by_the_side_move(gpu_ctx):
    """A batch, then bt_flow_track_side_move_device with rec_bytes = 128 behind a (crafted) expire that removes
    every third flow, then the sequence spaces go on under their new numbers."""
    ctx = gpu_ctx
    cap = 12
    conns = [tc.Conn(f, tc.M32 - 7 * f, 50 + f, sp=45000 + f) for f in range(cap)]
    first = tc.truth([c.seg(d, 0, 10) for c in conns for d in range(2)] + [c.seg(0, 10, 10) for c in conns])
    model, _, _ = run_case(ctx, tc.batches_of(first), cap, where="before")
    remap = np.array([0xFFFFFFFB if f % 3 == 0 else f - f // 3 - 1 for f in range(cap)], np.uint32)
    result = dict(n_flows_before=cap, n_flows=cap - 4, n_idle=4, n_expired=4, status=0)
    before = model.table
    want = before.copy()
    want_gone = str_.side_move(want, remap, result, 4)
    raw = abi.FlowTrackExpireResult(cap, cap - 4, 4, 4, 0)
    need = abi.flow_track_side_move_scratch_bytes(cap, REC)
    tab, gone, scratch = Guarded(ctx, REC * cap), Guarded(ctx, REC * 4), Guarded(ctx, need)
    d_remap, d_res = upload(ctx, remap), upload(ctx, np.frombuffer(bytes(raw), np.uint8))
    try:
        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, before.ctypes.data, REC * cap))
        ctx.flow_track_side_move(tab.ptr, REC, cap, d_remap.ptr, d_res.ptr, scratch.ptr, need, expired_side=gone.ptr, expired_cap=4)
        ctx.synchronize()
        moved = tab.read().view(tr.REC)
        assert moved.tobytes() == want.tobytes() and gone.read().tobytes() == want_gone.tobytes()
    finally:
        for x in (tab, gone, scratch, d_remap, d_res):
            x.free()
    live = [f for f in range(cap) if f % 3]
    second = [conns[f].seg(0, 15, 10) for f in live] + [conns[0].seg(0, 20, 10)]   # flow 0 came back as a new flow
    ids = [int(remap[f]) for f in live] + [cap - 4]
    _, got, results = run_case(ctx, [([r.frame for r in second], ids, [True] * len(ids), None)], cap, start=moved.copy(), where="after")
    assert [int(c) for c in got[0][0]] == [tc.OVERLAP] * len(live) + [tc.FIRST] and results[0]["old_bytes"] == 5 * len(live)


def test_an_empty_batch_still_writes_the_result(gpu_ctx):
    for cap in (0, 5):
        _, _, results = run_case(gpu_ctx, [([], [], [], None)], cap, where="empty")
        assert results[0] == dict(n=0, selected=0, seq_packets=0, first=0, in_order=0, gap=0, old=0, overlap=0, unkeyed=0, bad_ids=0,
                                  seq_bytes=0, old_bytes=0, gap_bytes=0)
