"""GPU: a payload pattern matched per flow and direction over the TCP segments in sequence order
(bt_flow_reasm_device, beatrice_amd/csrc/bt_flowreasm.hip). The kernels take flow_id and off directly: the
ids are crafted and the offsets come from bt_flow_tcpseq_host on the same frames. Every device call is
compared bit for bit with the host form (hit, rest, table, result) and with the restatement in
flowreasm_ref.py. The outputs, the table, the result and the scratch sit in poisoned buffers between two
256-byte guards; the scratch is filled with 0xA5 first and is exactly bt_flow_reasm_scratch_bytes long;
every call is made twice from the same starting table and the two runs must be byte-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowreasm_cases as rc  # noqa: E402
import flowreasm_ref as rr  # noqa: E402
import flowstat_ref as str_  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowreasm import bits_of, result_of, select_of  # noqa: E402
from test_flowstream import words_of  # noqa: E402
from test_gpu_flowstream import Frames, Pattern, upload  # noqa: E402
from test_gpu_flowtab import FORMATS, Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

BIDIR = 2
UNIT, CHUNK = 2048, 16384   # kFsUnit, kFsChunk
REC = 128


def device_once(ctx, pat, batch, n, d_ids, d_off, sel, flags, cap, tab_ptr, alias=None, stream=None, short=0):
    """One bt_flow_reasm_device into guarded outputs, a guarded result and a guarded scratch full of 0xA5.
    Returns (hit words, rest words, result dict)."""
    nw = (n + 63) // 64
    need = abi.flow_reasm_scratch_bytes(n, cap)
    hit, rest = Guarded(ctx, 8 * nw), Guarded(ctx, 8 * nw)
    res, scratch = Guarded(ctx, 64), Guarded(ctx, need)
    d_sel = None
    try:
        abi._check(abi.lib().bt_memset_d(ctx.h, scratch.ptr, 0xA5, need))
        if sel is not None and nw:
            if alias:
                abi._check(abi.lib().bt_memcpy_h2d(ctx.h, (hit if alias == "hit" else rest).ptr, sel.ctypes.data, 8 * nw))
            else:
                d_sel = upload(ctx, sel)
        ctx.synchronize()
        sel_ptr = None if sel is None or not nw else hit.ptr if alias == "hit" else rest.ptr if alias == "rest" else d_sel
        ctx.flow_reasm(batch, d_ids, sel_ptr, d_off, flags, pat.blob, pat.dev, tab_ptr if cap else None, cap, scratch.ptr if n else None,
                       need - short, res.ptr, hit=hit.ptr if nw else None, rest=rest.ptr if nw else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        scratch.read()   # its guards
        return hit.read(np.uint64), rest.read(np.uint64), abi.FlowReasmResult.from_bytes(res.read()).as_dict()
    finally:
        for g in (hit, rest, res, scratch, d_sel):
            if g is not None:
                g.free()


def run_case(ctx, pat, calls, cap, flags=BIDIR, fmt="packed", start=None, alias=None, stream=None, where=""):
    """calls: [rows]. Per call: the offsets by bt_flow_tcpseq_host, the restatement, the device call twice from the
    same table, the host form; the tables carry on. Returns (the restatement, [(hit bits, rest bits, result)])."""
    model = rr.Reasm(cap, pat.blob, flags, start)
    table = np.zeros(cap, rr.REC) if start is None else start.copy()
    seq_tab = np.zeros(cap, abi.FlowTcpseqRec)
    out = []
    for k, rows in enumerate(calls):
        at = f"{where} call {k}"
        n, nw = len(rows), (len(rows) + 63) // 64
        ids = np.ascontiguousarray([r.flow for r in rows], np.uint32)
        src = Frames(ctx, [r.frame for r in rows], fmt)
        sel = select_of(rows)
        if alias and sel is None:
            sel = words_of([True] * n)
        off = np.full(n, 7, np.int64)
        abi.flow_tcpseq_host(src.data, src.desc, ids, sel, flags, seq_tab, off=off)
        d_ids, d_off = upload(ctx, ids), upload(ctx, off)
        want_hit, want_rest, want_res = model.batch(src.seen, ids, off, sel)
        wtab = model.table
        runs = []
        try:
            for _ in range(2):
                tab = Guarded(ctx, REC * cap)
                try:
                    if cap:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, table.ctypes.data, REC * cap))
                    hit, rest, res = device_once(ctx, pat, src.batch, n, d_ids, d_off, sel, flags, cap, tab.ptr, alias, stream)
                    after = tab.read()
                finally:
                    tab.free()
                assert res["reserved0"] == 0 and res["reserved1"] == 0
                assert result_of(res) == want_res, f"{at}: result {result_of(res)} != {want_res}"
                bad = [i for i in range(n) if (int(hit[i >> 6]) ^ int(want_hit[i >> 6])) >> (i & 63) & 1]
                assert not bad and (hit == want_hit).all(), f"{at}: hit differs at packets {bad[:8]} (ids {ids[bad[:8]]})"
                assert (rest == want_rest).all(), f"{at}: rest"
                bad = np.nonzero((after.view(np.uint64).reshape(-1, 16) != wtab.view(np.uint64).reshape(-1, 16)).any(axis=1))[0]
                assert len(bad) == 0, f"{at}: table differs at flows {bad[:8]}: {after.view(rr.REC)[bad[:2]]} != {wtab[bad[:2]]}"
                runs.append((hit.tobytes(), rest.tobytes(), after.tobytes()))
            assert runs[0] == runs[1], f"{at}: two runs differ"
            if n:   # the host form, bit for bit
                host = table.copy().view(abi.FlowReasmRec)
                hhit, hrest = np.full(nw, 0xDEAD, np.uint64), np.full(nw, 0xDEAD, np.uint64)
                hres = abi.flow_reasm_host(src.data, src.desc, ids, sel, off, flags, pat.blob, host, hit=hhit, rest=hrest)
                assert result_of(hres) == want_res and (hhit.tobytes(), hrest.tobytes(), host.tobytes()) == runs[0], f"{at}: the host form"
        finally:
            for x in (src, d_ids, d_off):
                x.free()
        table = wtab.copy()
        out.append((bits_of(want_hit, n), bits_of(want_rest, n), want_res))
    return model, out


@pytest.fixture
def hello(gpu_ctx):
    pat = Pattern(gpu_ctx, rc.PATTERN)
    yield pat
    pat.free()


def test_the_named_cases(gpu_ctx, hello):
    """flowreasm_cases.crafted over two calls, with and without directions: swapped and reversed segments, trims,
    differing retransmits, holes filled in time and late, SYN and FIN, the wrap, a snapped frame, a far segment,
    both directions, what goes to rest, sentinels and bad ids."""
    calls, cap, _ = rc.crafted()
    _, out = run_case(gpu_ctx, hello, calls, cap, where="crafted")
    for rows, (hit, _, _) in zip(calls, out):
        assert [hit[i] for i, r in enumerate(rows) if r.hit is not None] == [r.hit for r in rows if r.hit is not None]
    run_case(gpu_ctx, hello, calls, cap, 0, where="crafted, one direction")


def test_the_gap_this_feature_closes(gpu_ctx, hello):
    """LO before HEL: the arrival-order matcher misses it, this call hits the first packet."""
    c = rc.Conn(0, 1000, 5000)
    _, out = run_case(gpu_ctx, hello, [[rc.seg(c, 0, 6, b"LOdef"), rc.seg(c, 0, 0, b"abcHEL")]], 1, where="swapped")
    assert out[0][0] == [True, False]


def test_a_64_position_pattern_whose_tail_spans_many_tiny_segments(gpu_ctx):
    pat = Pattern(gpu_ctx, rc.LONG)
    try:
        calls, cap = rc.long_pattern()
        _, out = run_case(gpu_ctx, pat, calls, cap, where="long")
        assert sum(out[0][0]) == 1
    finally:
        pat.free()


def tiny_stream(c, d, nseg, seed, window=8, reverse=False):
    """One direction of nseg one-to-three-byte segments with PATTERN planted, shuffled within windows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, nseg)
    s = bytearray(rng.choice(np.frombuffer(b"HELO.", np.uint8), int(lens.sum())).tobytes())
    for at in range(3, len(s) - 5, 37):
        s[at:at + 5] = rc.PATTERN.encode()
    rows, at = [], 0
    for ln in lens:
        rows.append(rc.seg(c, d, at, s[at:at + int(ln)]))
        at += int(ln)
    if reverse:
        return rows[::-1]
    out = []
    for k in range(0, nseg, window):
        part = rows[k:k + window]
        out += [part[j] for j in rng.permutation(len(part))]
    return out


def test_seventy_segments_of_one_stream_in_one_tile_in_reverse(gpu_ctx, hello):
    rows = tiny_stream(rc.Conn(0, 5, 9), 0, 70, 1, reverse=True)
    _, out = run_case(gpu_ctx, hello, [rows], 1, where="70 reversed")
    assert out[0][2]["stream_packets"] == 70 and out[0][2]["hit_packets"] >= 3 and out[0][2]["holes"] == 0


def test_streams_across_a_unit_and_a_chunk_of_the_sorted_list(gpu_ctx, hello):
    """One stream of 2,100 and one of 16,500 tiny segments, shuffled within windows of 8, interleaved in arrival."""
    a = tiny_stream(rc.Conn(0, rc.M32 - 100, 9, sp=41000), 0, UNIT + 52, 2)
    b = tiny_stream(rc.Conn(1, 77, 9, sp=41001), 0, CHUNK + 116, 3)
    rows = [r for pair in zip(a, b) for r in pair] + b[len(a):]
    _, out = run_case(gpu_ctx, hello, [rows], 2, where="unit and chunk")
    assert out[0][2]["stream_packets"] == len(rows) and out[0][2]["holes"] == 0 and out[0][2]["hit_packets"] > 500


def many(n, nflows, seed):
    """n packets over nflows flows: per flow short segments with a swap, a duplicate and a loss here and there."""
    rng = np.random.default_rng(seed)
    per = max(2, n // nflows)
    streams = []
    for f in range(nflows):
        c = rc.Conn(f, int(rng.integers(0, 1 << 32)), 7, sp=1024 + f % 60000)
        text = b"xxHELLOyyHELLO.." * (per // 2 + 1)
        rows, at = [], 0
        for k in range(per):
            ln = 1 + (f + k) % 7
            rows.append(rc.seg(c, (f >> 3) & 1 if nflows > 100 else 0, at, text[at:at + ln]))
            at += ln + (1 if (f + k) % 29 == 0 else 0)   # a loss
        op = f % 4
        if op == 1 and per > 1:
            rows[0], rows[1] = rows[1], rows[0]
        elif op == 2:
            rows.append(rows[0].again_data())
        streams.append(rows)
    if nflows <= 100:
        rows = [r for k in range(per) for s in streams for r in s[k:k + 1]] + [r for s in streams for r in s[per:]]
    else:
        rows = [r for s in streams for r in s]
    return rows[:n]


@pytest.mark.parametrize("nflows", [3, 20000])
def test_forty_thousand_packets(gpu_ctx, hello, nflows):
    rows = many(40000, nflows, nflows)
    _, out = run_case(gpu_ctx, hello, [rows], nflows, where=f"40000 over {nflows}")
    assert out[0][2]["stream_packets"] > 30000 and out[0][2]["holes"] > 0 and out[0][2]["hit_packets"] > 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes_at_tile_edges(gpu_ctx, hello, n):
    calls, _ = rc.random_calls(n, nflows=3, nbytes=200, ncalls=1, clean=False)
    rows = calls[0]
    while 0 < len(rows) < 2 * n:
        rows = rows + [r.again_data() for r in rows]
    _, out = run_case(gpu_ctx, hello, [rows[:n], rows[n:2 * n]], 3, where=f"n={n}")
    assert out[0][2]["n"] == n and out[1][2]["n"] == n


@pytest.mark.parametrize("cap", [1, 3, 257])
def test_flow_caps(gpu_ctx, hello, cap):
    calls, _ = rc.random_calls(cap, nflows=min(cap, 5), nbytes=500, ncalls=2, clean=False)
    if cap > 5:
        for rows in calls:
            for r in rows:
                r.flow = r.flow * 61 % cap if r.flow < cap else r.flow
    _, out = run_case(gpu_ctx, hello, calls, cap, where=f"cap={cap}")
    assert out[0][2]["hit_packets"] > 0


@pytest.mark.parametrize("alias", ["hit", "rest"])
def test_hit_and_rest_in_place_of_select(gpu_ctx, hello, alias):
    calls, cap, _ = rc.crafted()
    _, plain = run_case(gpu_ctx, hello, calls, cap, where="plain")
    _, same = run_case(gpu_ctx, hello, calls, cap, alias=alias, where=alias)
    assert plain == same


@pytest.mark.parametrize("fmt", FORMATS)
def test_three_calls_in_every_descriptor_format_on_a_stream_of_its_own(gpu_ctx, fmt):
    pat = Pattern(gpu_ctx, "GET|POST")
    st = gpu_ctx.stream_create()
    try:
        calls, _ = rc.random_calls(31, nflows=5, nbytes=900, ncalls=3, clean=False)
        _, out = run_case(gpu_ctx, pat, calls, 5, fmt=fmt, stream=st, where=fmt)
        assert sum(o[2]["late_packets"] for o in out) > 0 and sum(o[2]["holes"] for o in out) > 0
    finally:
        gpu_ctx.stream_destroy(st)
        pat.free()


def test_a_second_call_on_the_context_stream(gpu_ctx, hello):
    calls, truth = rc.random_calls(5, nflows=4, nbytes=2500, ncalls=2, clean=True)
    _, out = run_case(gpu_ctx, hello, calls, 4, where="two calls")
    assert out[1][2]["hit_packets"] > 0 and out[1][2]["holes"] == 0 and out[1][2]["late_packets"] == 0


def test_the_table_goes_through_a_device_expire_by_the_side_move(gpu_ctx, hello):
    """A call, then bt_flow_track_side_move_device with rec_bytes = 128 behind a (crafted) expire that removes every
    third flow, then the streams go on under their new numbers: HEL before the move, LO after it."""
    ctx = gpu_ctx
    cap = 12
    conns = [rc.Conn(f, rc.M32 - 7 * f, 50 + f, sp=45000 + f) for f in range(cap)]
    model, _ = run_case(ctx, hello, [[rc.seg(c, d, 0, b"xHEL") for c in conns for d in range(2)]], cap, where="before")
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
        moved = tab.read().view(rr.REC)
        assert moved.tobytes() == want.tobytes() and gone.read().tobytes() == want_gone.tobytes()
    finally:
        for x in (tab, gone, scratch, d_remap, d_res):
            x.free()
    live = [f for f in range(cap) if f % 3]
    second = [rc.seg(conns[f], 0, 4, b"LO") for f in live] + [rc.seg(conns[0], 0, 4, b"LO")]   # flow 0 came back as a new flow
    for r, f in zip(second, [int(remap[f]) for f in live] + [cap - 4]):
        r.flow = f
    # the sequence table moved as well: the offsets of the second call are those of the streams going on
    for r in second:
        r.key = None
    off = np.array([4] * len(live) + [0], np.int64)
    ids = np.array([r.flow for r in second], np.uint32)
    src = Frames(ctx, [r.frame for r in second], "packed")
    d_ids, d_off = upload(ctx, ids), upload(ctx, off)
    ref = rr.Reasm(cap, hello.blob, BIDIR, moved.copy())
    want_hit, _, want_res = ref.batch(src.seen, ids, off)
    tab = Guarded(ctx, REC * cap)
    try:
        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, moved.ctypes.data, REC * cap))
        hit, _, res = device_once(ctx, hello, src.batch, len(second), d_ids, d_off, None, BIDIR, cap, tab.ptr)
        assert tab.read().tobytes() == ref.table.tobytes() and (hit == want_hit).all() and result_of(res) == want_res
        assert bits_of(hit, len(second)) == [True] * len(live) + [False] and res["new_hit_flows"] == len(live)
    finally:
        for x in (tab, src, d_ids, d_off):
            x.free()


def test_a_scratch_one_byte_short_is_refused(gpu_ctx, hello):
    ctx = gpu_ctx
    rows = tiny_stream(rc.Conn(0, 5, 9), 0, 100, 4)
    src = Frames(ctx, [r.frame for r in rows], "packed")
    d_ids, d_off, tab = upload(ctx, np.zeros(100, np.uint32)), upload(ctx, np.zeros(100, np.int64)), Guarded(ctx, REC)
    try:
        with pytest.raises(abi.BtError, match="scratch_bytes"):
            device_once(ctx, hello, src.batch, 100, d_ids, d_off, None, BIDIR, 1, tab.ptr, short=1)
    finally:
        for x in (src, d_ids, d_off, tab):
            x.free()


def test_an_empty_batch_still_writes_the_result(gpu_ctx, hello):
    for cap in (0, 5):
        _, out = run_case(gpu_ctx, hello, [[]], cap, where="empty")
        assert out[0][2] == {k: 0 for k in rr.RESULT}
