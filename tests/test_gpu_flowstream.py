"""GPU: a payload pattern matched per flow and direction across packet boundaries
(bt_flow_stream_device, beatrice_amd/csrc/bt_flowstream.hip). The kernels take flow_id directly, so the
ids are crafted. Every device call is compared bit for bit with the host form (hit words, table,
result) and with the restatement in flowstream_ref.py (streams as Python bytes, matches by `re`), never
with anything derived from the code under test. The hit words, the table, the result and the scratch
sit in poisoned buffers between two 256-byte guards; the scratch is filled with 0xA5 first; every call
is made twice from the same starting table and the two runs must be byte-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import flowstat_ref as str_  # noqa: E402
import flowstream_cases as fc  # noqa: E402
import flowstream_ref as sr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowstream import lay_out, words_of  # noqa: E402
from test_gpu_flowtab import FORMATS, Guarded, Source  # noqa: E402

pytestmark = pytest.mark.gpu

BIDIR = 2
UNIT, CHUNK = 2048, 16384   # kFsUnit, kFsChunk
REC = 32


def upload(ctx, arr):
    d = ctx.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        d.upload(arr)
    return d


class Frames:
    """Crafted frames on the device in one of the three formats, and as the call sees them: at a fixed
    stride every frame is zero-padded to the stride, which is then its length."""

    def __init__(self, ctx, frames, fmt):
        self.n, self.d_data, self.d_desc = len(frames), None, None
        if fmt == "stride":
            stride = (max([len(f) for f in frames] + [64]) + 15) // 16 * 16
            self.seen = [bytes(f) + bytes(stride - len(f)) for f in frames]
            self.data = np.frombuffer(b"".join(self.seen) + bytes(64), np.uint8)
            self.desc = np.array([i * stride | stride << 48 for i in range(self.n)], np.uint64)   # the host form's view
            self.d_data = ctx.alloc(len(self.data) + 256)
            self.d_data.zero()
            self.d_data.upload(self.data)
            self.batch = abi.Batch(self.d_data.ptr, None, stride, self.n, 0, 0, 0)
            self.src = None
            return
        self.seen = [bytes(f) for f in frames]
        self.data, self.desc = lay_out(frames)
        self.src = Source(ctx, "c3", self.n, fmt, data=self.data, desc=self.desc if self.n else np.zeros(1, np.uint64))
        self.batch = self.src.batch

    def free(self):
        if self.src is not None:
            self.src.free()
        if self.d_data is not None:
            self.d_data.free()


class Pattern:
    def __init__(self, ctx, pattern):
        self.text = pattern
        self.blob, self.info = abi.flow_stream_compile(pattern)
        self.dev = upload(ctx, self.blob)

    def free(self):
        self.dev.free()


def device_once(ctx, pat, batch, n, d_ids, sel, flags, cap, tab_ptr, want_hit=True, in_place=False, stream=None):
    """One bt_flow_stream_device into guarded hit words, a guarded result and a guarded scratch full of 0xA5.
    Returns (hit words or None, result dict)."""
    nw = (n + 63) // 64
    need = abi.flow_stream_scratch_bytes(n, cap)
    hit = Guarded(ctx, 8 * nw) if want_hit or in_place else None
    res, scratch = Guarded(ctx, 64), Guarded(ctx, need)
    d_sel = None
    try:
        abi._check(abi.lib().bt_memset_d(ctx.h, scratch.ptr, 0xA5, need))
        if sel is not None and nw:
            if in_place:
                abi._check(abi.lib().bt_memcpy_h2d(ctx.h, hit.ptr, sel.ctypes.data, 8 * nw))
            else:
                d_sel = upload(ctx, sel)
        ctx.synchronize()
        sel_ptr = None if sel is None or not nw else hit.ptr if in_place else d_sel
        ctx.flow_stream(batch, d_ids, sel_ptr, flags, pat.blob, pat.dev, tab_ptr if cap else None, cap, scratch.ptr if n else None, need,
                        res.ptr, hit=hit.ptr if hit and nw else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        scratch.read()   # its guards
        out = abi.FlowStreamResult.from_bytes(res.read()).as_dict()
        assert out.pop("reserved") == [0] * 7
        return (hit.read(np.uint64) if hit else None), out
    finally:
        for g in (hit, res, scratch, d_sel):
            if g is not None:
                g.free()


def run_case(ctx, pat, batches, cap, flags=0, fmt="packed", start=None, in_place=False, stream=None, where="", want_hits=True):
    """batches: [(frames, ids, select bits)]. Per batch: the restatement, the device call twice from the same
    table, the host form; the table carries on. Returns (the restatement, [hit words], [result])."""
    model = sr.Streams(cap, pat.text, pat.blob, flags, start)
    table = np.zeros(cap, sr.STREAM_REC) if start is None else start.copy()
    hits, results = [], []
    for k, (frames, ids, bits) in enumerate(batches):
        at = f"{where} batch {k}"
        n, ids = len(frames), np.ascontiguousarray(ids, np.uint32)
        src = Frames(ctx, frames, fmt)
        d_ids = upload(ctx, ids)
        sel = None if all(bits) and not in_place else words_of(bits)
        if sel is not None and n % 64:
            sel[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
        want_hit, want_res = model.batch(src.seen, ids, sel)
        runs = []
        try:
            for _ in range(2):
                tab = Guarded(ctx, REC * cap)
                try:
                    if cap:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, table.ctypes.data, REC * cap))
                    hit, res = device_once(ctx, pat, src.batch, n, d_ids, sel, flags, cap, tab.ptr, want_hits, in_place, stream)
                    after = tab.read()
                finally:
                    tab.free()
                assert res == want_res, f"{at}: result {res} != {want_res}"
                if hit is None:   # not asked for: the table and the result are the same
                    hit = want_hit
                bad = [i for i in range(n) if (int(hit[i >> 6]) ^ int(want_hit[i >> 6])) >> (i & 63) & 1]
                assert not bad and (hit == want_hit).all(), f"{at}: hit differs at packets {bad[:8]} (ids {ids[bad[:8]]})"
                rows = np.nonzero((after.view(np.uint64).reshape(-1, 4) != model.table.view(np.uint64).reshape(-1, 4)).any(axis=1))[0]
                assert len(rows) == 0, f"{at}: table differs at flows {rows[:8]}: {after.view(sr.STREAM_REC)[rows[:4]]} != {model.table[rows[:4]]}"
                runs.append((hit.tobytes(), after.tobytes()))
            assert runs[0] == runs[1], f"{at}: two runs differ"
            if n:   # the host form, bit for bit
                host = table.copy().view(abi.FlowStreamRec)
                hhit = np.full((n + 63) // 64, 0xDEAD, np.uint64)
                hres = abi.flow_stream_host(src.data, src.desc, ids, sel, flags, pat.blob, host, hit=hhit)
                hres.pop("reserved")
                assert hres == want_res and hhit.tobytes() == runs[0][0] and host.tobytes() == runs[0][1], f"{at}: the host form"
        finally:
            src.free()
            d_ids.free()
        table = model.table.copy()
        hits.append(want_hit)
        results.append(want_res)
    return model, hits, results


@pytest.mark.parametrize("flags", [0, BIDIR])
@pytest.mark.parametrize("k", range(len(fc.PATTERNS)), ids=[p[0] for p in fc.PATTERNS])
def test_the_named_cases_of_every_pattern(gpu_ctx, k, flags):
    """flowstream_cases.crafted: a match split at every cut point, over three packets and over one packet per
    byte (T hops back to the head of the list), ending on a packet's first and last byte, across the
    piece boundaries, wholly in the tail; the halves interleaved with the other direction, pure ACKs,
    other flows and unselected packets; in two flows, two directions, two batches; UDP, IP options,
    IPv6, a VLAN tag, Ethernet padding, a snapped frame; every payload length; sentinels and bad ids."""
    pattern, positions, text = fc.PATTERNS[k]
    pat = Pattern(gpu_ctx, pattern)
    try:
        assert pat.info["positions"] == positions
        rows, cap = fc.crafted(text, pat.info["tail"])
        _, _, results = run_case(gpu_ctx, pat, fc.batches_of(rows), cap, flags, fmt=FORMATS[(k + flags) % 3], where=pattern)
        assert results[0]["hit_packets"] >= len(text) - 1 and results[0]["bad_ids"] == 1 and results[0]["unkeyed"] == 4
        assert results[1]["hit_packets"] > 8 and results[1]["new_hit_flows"] >= 8
    finally:
        pat.free()


def test_the_gap_this_feature_closes(gpu_ctx):
    """Why stream matching exists. GE + T / in two TCP segments: the per-packet PAYLOAD filter (program
    payload:GET through bt_parse_filter_device) passes neither packet, because neither holds the match;
    the stream matcher hits the second, where the match ends. Without bt_flow_stream_device this fails."""
    from pcap_filter import parse_filter
    frames = [fc.frame(b"GE"), fc.frame(b"T / HTTP/1.1\r\n"), fc.frame(b"GET / HTTP/1.1\r\n", sp=40001)]
    ctx = abi.Context(0)   # a program of its own: the shared context's stays as it is
    try:
        src = Frames(ctx, frames, "packed")
        ver = Guarded(ctx, 8)
        pat = Pattern(ctx, "GET")
        try:
            slots = ctx.compile([parse_filter("payload:GET")])
            assert all(s.kind != 9 for s in slots)   # decided on the GPU
            ctx.reserve(3)
            ctx.run_device(src.batch, abi.Outputs(None, 0, ver.ptr, None, None, None))
            ctx.synchronize()
            assert int(ver.read(np.uint64)[0]) & 7 == 0b100, "the per-packet filter sees no match in either segment, and the whole one"
            _, hits, _ = run_case(ctx, pat, [(frames, [0, 0, 1], [True] * 3)], 2, where="gap")
            assert int(hits[0][0]) == 0b110
        finally:
            for x in (src, ver, pat):
                x.free()
    finally:
        ctx.close()


def test_a_match_in_the_tail_does_not_hit_again(gpu_ctx):
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        frames = [fc.frame(b"..POST"), fc.frame(b"x"), fc.frame(b"PO"), fc.reply(b"ST"), fc.frame(b"ST")]
        for flags, want in ((0, 0b01001), (BIDIR, 0b10001)):   # without directions the reply completes it
            _, hits, _ = run_case(gpu_ctx, pat, [(frames, [0] * 5, [True] * 5)], 1, flags, where="tail")
            assert int(hits[0][0]) == want
        # halves in opposite directions meet only in a table without directions
        frames = [fc.frame(b"PO"), fc.reply(b"ST"), fc.frame(b"!")]
        for flags, want in ((0, 0b010), (BIDIR, 0)):
            _, hits, _ = run_case(gpu_ctx, pat, [(frames, [0] * 3, [True] * 3)], 1, flags, where="directions")
            assert int(hits[0][0]) == want
    finally:
        pat.free()


def mixed_batch(n, seed, text, nflows, lens=(0, 1, 2, 3, 5, 9)):
    rng = np.random.default_rng(seed)
    pool = [(mk, int(ln), int(v)) for mk in (fc.frame, fc.reply) for ln in lens for v in range(3)]
    made = {p: p[0](fc.filler(p[1], text, 31 * p[1] + p[2])) for p in pool}
    pick = rng.integers(0, len(pool), n)
    frames = [made[pool[j]] for j in pick]
    ids = rng.integers(0, nflows, n).astype(np.uint32)
    ids[rng.integers(0, n, 1 + n // 50)] = 0xFFFFFFFE
    ids[rng.integers(0, n, 1 + n // 90)] = nflows + 5
    return frames, ids, [bool(x) for x in rng.integers(0, 5, n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, UNIT - 1, UNIT, UNIT + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_sizes_at_tile_unit_and_chunk_edges(gpu_ctx, n):
    """Short payloads over 40 flows in two directions, so that most matches cross packets; two batches."""
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        batches = [mixed_batch(n, n, b"POST", 40), mixed_batch(n, n + 1, b"GET", 40)]
        _, _, results = run_case(gpu_ctx, pat, batches, 40, BIDIR, where=f"n={n}")
        assert results[0]["n"] == n
        if n >= UNIT:
            assert results[1]["hit_packets"] > 10 and results[0]["bad_ids"] > 0 and results[0]["unkeyed"] > 0
    finally:
        pat.free()


@pytest.mark.parametrize("cap", [127, 128, 129, 32767, 32768, 32769])
def test_flow_caps_on_both_sides_of_the_sort_digit_boundaries(gpu_ctx, cap):
    """The sort key is flow << 1 | direction: 2 * cap crosses 2^8 and 2^16. The ids hold 0, cap - 1, the
    boundary values and cap (a bad id)."""
    pat = Pattern(gpu_ctx, "colou?r")
    try:
        frames, ids, bits = mixed_batch(700, cap, b"color", cap, lens=(1, 2, 3, 4))
        ids, bits = list(ids), list(bits)
        ids[5] = cap
        edge = sorted({0, cap - 1, cap // 2, cap // 2 - 1, 63, 64, 126, min(128, cap - 1)})
        for part in (b"xco", b"l", b"o", b"r!"):   # behind the noise, every edge flow gets a match over four packets, round robin
            for v in edge:
                frames.append((fc.frame if v % 2 else fc.reply)(part))
                ids.append(v)
                bits.append(True)
        model, _, results = run_case(gpu_ctx, pat, [(frames, ids, bits), (frames[::-1], ids[::-1], bits[::-1])], cap, BIDIR, where=f"cap={cap}")
        assert results[0]["bad_ids"] >= 1 and results[0]["hit_packets"] >= len(edge) and int(model.table["hit_packets"][cap - 1].sum()) > 0
    finally:
        pat.free()


@pytest.mark.parametrize("fmt", FORMATS)
def test_descriptor_formats_on_a_stream_of_its_own(gpu_ctx, fmt):
    pat = Pattern(gpu_ctx, "Host: example\\.com")
    st = gpu_ctx.stream_create()
    try:
        batches = [mixed_batch(UNIT + 70, 3, b"Host: example.com", 9, lens=(0, 1, 4, 11, 30))]
        _, _, results = run_case(gpu_ctx, pat, batches, 9, BIDIR, fmt=fmt, stream=st, where=fmt)
        assert results[0]["hit_packets"] > 3
    finally:
        gpu_ctx.stream_destroy(st)
        pat.free()


def test_hit_in_place_of_select(gpu_ctx):
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        _, _, results = run_case(gpu_ctx, pat, [mixed_batch(CHUNK + 300, 8, b"POST", 17)], 17, 0, in_place=True, where="in place")
        assert 0 < results[0]["hit_packets"] < results[0]["selected"] < CHUNK + 300
    finally:
        pat.free()


def test_without_the_hit_words(gpu_ctx):
    """hit is optional: the table, the counts and the first hits are the same without it."""
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        batches = [mixed_batch(UNIT + 5, 21, b"POST", 11), mixed_batch(UNIT + 5, 22, b"GET", 11)]
        _, _, results = run_case(gpu_ctx, pat, batches, 11, BIDIR, want_hits=False, where="no hit words")
        assert results[0]["hit_packets"] > 0 and results[0]["new_hit_flows"] > 0
    finally:
        pat.free()


def test_a_frame_at_the_descriptors_16_bit_limit(gpu_ctx):
    """65,535 frame bytes: 512 pieces of one packet, a match across the last piece boundary and one that the
    next packet completes."""
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        room = 65535 - len(fc.frame(b""))
        body = bytearray(fc.filler(room, b"POST", 2))
        body[511 * 128 - 2:511 * 128 + 2] = b"POST"
        body[-2:] = b"GE"
        frames = [fc.frame(b"PO"), fc.frame(bytes(body)), fc.frame(b"T")]
        assert len(frames[1]) == 65535
        _, hits, results = run_case(gpu_ctx, pat, [(frames, [0, 0, 0], [True] * 3)], 1, where="64k")
        assert int(hits[0][0]) & 0b100 and results[0]["stream_bytes"] == room + 3
    finally:
        pat.free()


def test_a_starting_table_with_a_state_and_wrapping_counts(gpu_ctx):
    """d holds any bits of the pattern's positions: streams that reach the head of their list go on from it,
    the others have forgotten it by their T-th byte."""
    pattern, positions, text = fc.PATTERNS[5]
    pat = Pattern(gpu_ctx, pattern)
    try:
        rng = np.random.default_rng(5)
        start = np.zeros(8, sr.STREAM_REC)
        start["d"] = rng.integers(0, 1 << positions, (8, 2), dtype=np.uint64)
        start["hit_packets"][::2, 0] = 3
        start["stream_packets"][:] = 0xFFFFFFFF
        frames = [fc.frame(text[k:]) for k in range(8)] + [fc.reply(text[k + 20:]) for k in range(8)] + [fc.frame(text)] * 8
        model, _, results = run_case(gpu_ctx, pat, [(frames, list(range(8)) * 3, [True] * 24)], 8, BIDIR, start=start, where="state")
        assert int(model.table["stream_packets"][0][0]) == 1 and results[0]["new_hit_flows"] <= 4
    finally:
        pat.free()


def test_the_table_goes_through_a_device_expire_by_the_side_move(gpu_ctx):
    """A batch, then bt_flow_track_side_move_device with rec_bytes = 32 behind a (crafted) expire that removes
    every third flow, then the streams go on under their new numbers: a match whose first half lies
    before the expire ends behind it."""
    ctx = gpu_ctx
    pat = Pattern(ctx, "GET|POST")
    cap = 12
    try:
        first = [fc.frame(b"PO", sp=1000 + f) for f in range(cap)]
        model, _, _ = run_case(ctx, pat, [(first, list(range(cap)), [True] * cap)], cap, where="before")
        remap = np.array([0xFFFFFFFB if f % 3 == 0 else f - f // 3 - 1 for f in range(cap)], np.uint32)
        result = dict(n_flows_before=cap, n_flows=cap - 4, n_idle=4, n_expired=4, status=0)
        want = model.table.copy()
        want_gone = str_.side_move(want, remap, result, 4)
        raw = abi.FlowTrackExpireResult(cap, cap - 4, 4, 4, 0)
        need = abi.flow_track_side_move_scratch_bytes(cap, REC)
        tab, gone, scratch = Guarded(ctx, REC * cap), Guarded(ctx, REC * 4), Guarded(ctx, need)
        d_remap, d_res = upload(ctx, remap), upload(ctx, np.frombuffer(bytes(raw), np.uint8))
        try:
            abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, model.table.ctypes.data, REC * cap))
            ctx.flow_track_side_move(tab.ptr, REC, cap, d_remap.ptr, d_res.ptr, scratch.ptr, need, expired_side=gone.ptr, expired_cap=4)
            ctx.synchronize()
            moved = tab.read().view(sr.STREAM_REC)
            assert moved.tobytes() == want.tobytes() and gone.read().tobytes() == want_gone.tobytes()
        finally:
            for x in (tab, gone, scratch, d_remap, d_res):
                x.free()
        live = [f for f in range(cap) if f % 3]
        second = [fc.frame(b"ST", sp=1000 + f) for f in live] + [fc.frame(b"ST", sp=1000)]   # flow 0 came back as a new flow
        ids = [int(remap[f]) for f in live] + [cap - 4]
        _, hits, results = run_case(ctx, pat, [(second, ids, [True] * len(ids))], cap, start=moved.copy(), where="after")
    finally:
        pat.free()
    # run_case's restatement took the moved table's states as they are: every survivor completes its match
    assert int(hits[0][0]) == (1 << len(live)) - 1 and results[0]["new_hit_flows"] == len(live)


def test_an_empty_batch_still_writes_the_result(gpu_ctx):
    pat = Pattern(gpu_ctx, "GET|POST")
    try:
        for cap in (0, 5):
            _, _, results = run_case(gpu_ctx, pat, [([], [], [])], cap, where="empty")
            assert results[0] == dict(n=0, selected=0, stream_packets=0, hit_packets=0, unkeyed=0, bad_ids=0, stream_bytes=0, new_hit_flows=0)
    finally:
        pat.free()
