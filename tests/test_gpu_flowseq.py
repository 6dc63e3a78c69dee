"""GPU: a packet's position inside its flow and the per-flow cut-off (bt_flow_seq_device,
beatrice_amd/csrc/bt_flowseq.hip). The kernels take flow_id directly, so the ids are crafted. Expected
values come from the restatement in flowseq_ref.py (a plain loop over the packets), never from the
code under test; the host form must agree bit for bit. Every output, the table, the result and the
scratch sit in poisoned buffers between two 256-byte guards; the scratch is filled with 0xA5 first;
every call is made twice and the two runs must be byte-equal."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowseq_ref as qr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import FORMATS, POISON, Guarded, Source, golden_keys, select_words  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 3 * 16384 + 17
SIZES = [0, 1, 63, 64, 65, 16384, 16385, BIG]
CAPS = [1, 2, 64, 65, 256, 257, 4096, 4097, 65536, 65537, (1 << 24) + 1]
SENTINELS = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD], np.uint32)   # UNSELECTED, NONE, OVERFLOW
LIMITS = [(0, 0), (1, 0), (3, 0), (0, 1), (0, 200), (3, 200)]
SEQ, OFF, SEL = 1, 2, 4


def upload(ctx, arr):
    d = ctx.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        d.upload(arr)
    return d


def lengths(n):
    return 60 + (np.arange(n, dtype=np.int64) * 7) % 1400


def crafted_source(ctx, n, fmt, lens=None):
    """Descriptors with the caller's lengths (no frame byte is read); at a fixed stride every length is the stride."""
    if fmt == "stride":
        return Source(ctx, "edge", n, fmt)
    lens = lengths(n) if lens is None else np.asarray(lens, np.int64)
    desc = ((np.arange(n, dtype=np.uint64) % np.uint64(64)) * np.uint64(64)) | (lens.astype(np.uint64) << np.uint64(48))
    return Source(ctx, "edge", n, fmt, data=np.zeros(4096, np.uint8), desc=desc)


def device_once(ctx, batch, n, d_ids, sel, cap, tab_ptr, mp, mb, flags, outs, in_place=False, stream=None):
    """One bt_flow_seq_device into guarded outputs, a guarded result and a guarded scratch full of 0xA5.
    Returns (seq, byte_off, out words, result dict), None for an output that was not asked for."""
    nw = (n + 63) // 64
    need = abi.flow_seq_scratch_bytes(n, cap)
    seq = Guarded(ctx, 4 * n) if outs & SEQ else None
    off = Guarded(ctx, 8 * n) if outs & OFF else None
    out = Guarded(ctx, 8 * nw) if outs & SEL or in_place else None
    res, scratch = Guarded(ctx, 64), Guarded(ctx, need)
    d_sel = None
    try:
        if need:
            abi._check(abi.lib().bt_memset_d(ctx.h, scratch.ptr, 0xA5, need))
        if sel is not None and nw:
            if in_place:
                abi._check(abi.lib().bt_memcpy_h2d(ctx.h, out.ptr, sel.ctypes.data, 8 * nw))
            else:
                d_sel = upload(ctx, sel)
        ctx.synchronize()
        sel_ptr = None if sel is None or not nw else out.ptr if in_place else d_sel
        ctx.flow_seq(batch, d_ids, sel_ptr, tab_ptr if cap else None, cap, scratch.ptr if n else None, need, res.ptr,
                     max_packets=mp, max_bytes=mb, flags=flags, seq=seq.ptr if seq and n else None, byte_off=off.ptr if off and n else None,
                     out_select=out.ptr if out and nw else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        scratch.read()   # its guards
        return (seq.read(np.uint32) if seq else None, off.read(np.uint64) if off else None, out.read(np.uint64) if out else None,
                abi.FlowSeqResult.from_bytes(res.read()).as_dict())
    finally:
        for g in (seq, off, out, res, scratch, d_sel):
            if g is not None:
                g.free()


def run_case(ctx, ids, cap, sel=None, mp=0, mb=0, flags=0, outs=SEQ | OFF | SEL, start=None, fmt="packed", in_place=False,
             stream=None, lens=None, where=""):
    """The restatement, then the device call twice from the same starting table (both runs byte-equal and
    equal to the restatement, the table between its guards included), then the host form. Returns the
    restatement's (seq, byte_off, words, result, table)."""
    ids = np.ascontiguousarray(ids, np.uint32)
    n = len(ids)
    src = crafted_source(ctx, n, fmt, lens)
    d_ids = upload(ctx, ids)
    first = np.zeros(cap, qr.SEQ_REC) if start is None else start
    want = first.copy()
    wseq, woff, wout, wres = qr.number(want, ids, src.lens, sel, mp, mb, flags)
    runs = []
    try:
        for _ in range(2):
            tab = Guarded(ctx, 16 * cap)
            try:
                if cap:
                    abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, first.ctypes.data, 16 * cap))
                seq, off, out, res = device_once(ctx, src.batch, n, d_ids, sel, cap, tab.ptr, mp, mb, flags, outs, in_place, stream)
                table = tab.read()
            finally:
                tab.free()
            assert res == wres, f"{where}: result {res} != {wres}"
            if seq is not None:
                bad = np.nonzero(seq != wseq)[0]
                assert len(bad) == 0, f"{where}: seq differs at {bad[:8]}: {seq[bad[:8]]} != {wseq[bad[:8]]} (ids {ids[bad[:8]]})"
            if off is not None:
                bad = np.nonzero(off != woff)[0]
                assert len(bad) == 0, f"{where}: byte_off differs at {bad[:8]}: {off[bad[:8]]} != {woff[bad[:8]]}"
            if out is not None:
                bad = np.nonzero(out != wout)[0]
                assert len(bad) == 0, f"{where}: out_select differs at words {bad[:8]}: {out[bad[:8]]} != {wout[bad[:8]]}"
            bad = np.nonzero(table.view(np.uint64) != want.view(np.uint64).reshape(-1))[0]
            assert len(bad) == 0, f"{where}: table differs at records {bad[:8] // 2}"
            runs.append(tuple(None if x is None else x.tobytes() for x in (seq, off, out, table)))
        assert runs[0] == runs[1], f"{where}: two runs differ"
        if fmt != "stride" and n:   # the host form, bit for bit
            host = first.copy().view(abi.FlowSeqRec)
            hseq, hoff, hout = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros((n + 63) // 64, np.uint64)
            hres = abi.flow_seq_host(src.desc, ids, sel, host, mp, mb, flags, seq=hseq, byte_off=hoff, out_select=hout)
            assert hres == wres and host.tobytes() == runs[0][3], f"{where}: the host form"
            assert (hseq == wseq).all() and (hoff == woff).all() and (hout == wout).all(), f"{where}: the host form's outputs"
    finally:
        src.free()
        d_ids.free()
    return wseq, woff, wout, wres, want


@functools.lru_cache(maxsize=None)
def pattern(name, n=BIG):
    """(ids, flow_cap) of an id pattern at n packets."""
    rng = np.random.default_rng(len(name) * 1000 + n)
    i = np.arange(n, dtype=np.uint32)
    if name == "one":
        return np.zeros(n, np.uint32), 1
    if name == "own":
        return i, n
    if name == "reversed":
        return (n - 1 - i).astype(np.uint32), n
    if name == "two":
        return (i & 1).astype(np.uint32), 2
    if name == "37":
        return rng.integers(0, 37, n).astype(np.uint32), 37
    if name == "skewed":
        ids = np.where(rng.integers(0, 2, n) == 0, 4999, rng.integers(0, 5000, n)).astype(np.uint32)
        return ids, 5000
    assert name == "mixed"
    ids = rng.integers(0, 300, n).astype(np.uint32)
    kind = rng.integers(0, 8, n)
    ids[kind == 0] = SENTINELS[rng.integers(0, 3, int((kind == 0).sum()))]
    ids[kind == 1] = 300 + rng.integers(0, 1 << 20, int((kind == 1).sum())).astype(np.uint32)
    return ids, 300


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    """37 flows with sentinels and bad ids mixed in; the format, the selection and the flag rotate."""
    si = SIZES.index(n)
    ids, cap = pattern("mixed", n)
    sel = select_words(("random", "null", "ones")[si % 3], n)
    _, _, _, res, _ = run_case(gpu_ctx, ids, cap, sel, 3, 2000, si % 2, fmt=FORMATS[si % 3], where=f"n={n}")
    assert res["n"] == n and res["selected"] == res["numbered"] + res["unkeyed"] + res["bad_ids"]
    if n >= 16384:
        assert res["numbered"] > res["kept"] - res["unkeyed"] * (si % 2) > 0 and res["bad_ids"] > 0


@pytest.mark.parametrize("name", ["one", "own", "reversed", "two", "37", "skewed", "mixed"])
def test_id_patterns_at_the_largest_size(gpu_ctx, name):
    """One flow spans every chunk of the sorted list; every packet its own flow, ascending and descending;
    two flows alternating; few flows; a skewed draw; sentinels and bad ids."""
    ids, cap = pattern(name)
    _, _, _, res, table = run_case(gpu_ctx, ids, cap, None, 3, 0, qr.KEEP_UNKEYED, where=name)
    assert res["flows"] == len(np.unique(ids[ids < cap])) == res["new_flows"] and int(table["packets"].sum()) == res["numbered"]
    if name == "one":
        assert res["kept"] == 3 and int(table["packets"][0]) == BIG
    if name in ("own", "reversed"):
        assert res["kept"] == BIG == res["flows"]


@pytest.mark.parametrize("cap", CAPS)
def test_flow_caps_on_both_sides_of_every_digit_boundary(gpu_ctx, cap):
    """Ids over the whole of [0, cap) with the edges in: 0, cap - 1, cap (a bad id), and for 2^24 + 1 the ids
    2^24 - 1 and 2^24. The table starts non-zero."""
    n = BIG if cap <= 65537 else 16385
    rng = np.random.default_rng(cap)
    ids = rng.integers(0, cap, n).astype(np.uint32)
    ids[rng.integers(0, n, 200)] = cap - 1
    ids[rng.integers(0, n, 200)] = 0
    ids[rng.integers(0, n, 50)] = cap
    for k, edge in enumerate((1 << 6, 1 << 8, 1 << 12, 1 << 16, 1 << 18, 1 << 24)):
        for v in (edge - 1, edge):
            if v < cap:
                ids[rng.integers(0, n, 20)] = v
    start = np.zeros(cap, qr.SEQ_REC)
    start["packets"][::3] = 2
    start["bytes"][::3] = 150
    _, _, _, res, _ = run_case(gpu_ctx, ids, cap, select_words("random", n), 4, 0, 0, start=start, where=f"cap={cap}")
    assert res["bad_ids"] > 0 and res["flows"] > res["new_flows"] >= (cap > 2)


@pytest.mark.parametrize("kind", ["null", "zeros", "every_other", "one_percent", "ones", "in_place"])
def test_select(gpu_ctx, kind):
    ids, cap = pattern("skewed")
    n = BIG
    if kind == "every_other":
        sel = np.full((n + 63) // 64, 0x5555555555555555, np.uint64)
    elif kind == "one_percent":
        sel = fr.pack_bits(np.random.default_rng(3).integers(0, 100, n) == 0)
    else:
        sel = select_words("random" if kind == "in_place" else kind, n)   # ones: garbage bits at or above n
    _, _, _, res, _ = run_case(gpu_ctx, ids, cap, sel, 2, 0, 0, in_place=kind == "in_place", where=kind)
    want = {"null": n, "zeros": 0, "every_other": (n + 1) // 2, "ones": n}.get(kind)
    assert want is None or res["selected"] == want
    assert kind != "one_percent" or 300 < res["selected"] < 700


@pytest.mark.parametrize("flags", [0, qr.KEEP_UNKEYED])
@pytest.mark.parametrize("mp,mb", LIMITS)
def test_limits(gpu_ctx, mp, mb, flags):
    ids, cap = pattern("mixed")
    _, _, _, res, _ = run_case(gpu_ctx, ids, cap, None, mp, mb, flags, where=f"limits {mp} {mb} {flags}")
    unk = res["unkeyed"] if flags else 0
    if (mp, mb) == (0, 0):
        assert res["kept"] == res["numbered"] + unk and res["kept_bytes"] == res["numbered_bytes"]
    else:
        assert res["flows"] <= res["kept"] - unk < res["numbered"]
        if mp == 1 or mb == 1:
            assert res["kept"] - unk == res["flows"] == cap


@pytest.mark.parametrize("outs", range(8))
def test_every_subset_of_the_outputs(gpu_ctx, outs):
    """Each of seq, byte_off and out_select alone, together, and none: the table and the result are the same."""
    ids, cap = pattern("mixed", 16385)
    _, _, _, res, _ = run_case(gpu_ctx, ids, cap, select_words("random", 16385), 3, 0, qr.KEEP_UNKEYED, outs=outs, where=f"outs={outs}")
    assert res["kept"] > res["unkeyed"] > 0   # computed with and without out_select


@pytest.mark.parametrize("kind", ["zero", "random", "saturated"])
def test_starting_tables(gpu_ctx, kind):
    """saturated: packets = 0xFFFFFFFD and bytes near 2^40: seq saturates while the cut-off decides on 64 bits."""
    ids, cap = pattern("37")
    start = np.zeros(cap, qr.SEQ_REC)
    mp, mb = 3, 0
    if kind == "random":
        rng = np.random.default_rng(11)
        start["packets"], start["bytes"] = rng.integers(0, 5, cap), rng.integers(0, 1 << 50, cap)
    if kind == "saturated":
        start["packets"], start["bytes"] = 0xFFFFFFFD, (1 << 40) - 3000
        mp, mb = (1 << 32) + 2, (1 << 40)
    seq, off, out, res, table = run_case(gpu_ctx, ids, cap, None, mp, mb, 0, start=start, where=kind)
    if kind == "saturated":
        assert int((seq == qr.SEQ_MAX).sum()) == BIG - cap and int((seq == 0xFFFFFFFD).sum()) == cap
        assert cap < res["kept"] <= 5 * cap and int(table["packets"].max()) > 1 << 32 and res["new_flows"] == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_descriptor_formats_on_a_stream_of_its_own(gpu_ctx, fmt):
    ids, cap = pattern("skewed", 16385 + 64)
    st = gpu_ctx.stream_create()
    try:
        _, _, _, res, _ = run_case(gpu_ctx, ids, cap, select_words("random", len(ids)), 0, 3000, 0, fmt=fmt, stream=st, where=fmt)
        assert 0 < res["kept"] < res["numbered"]
    finally:
        gpu_ctx.stream_destroy(st)


def test_lengths_at_the_16_bit_limit_and_zero(gpu_ctx):
    n = 16385
    lens = np.where(np.arange(n) % 5 == 0, 65535, np.where(np.arange(n) % 7 == 0, 0, 1500))
    ids, cap = pattern("two", n)
    _, off, _, res, table = run_case(gpu_ctx, ids, cap, None, 0, 1 << 20, 0, fmt="xdp", lens=lens, where="long frames")
    assert int(table["bytes"].sum()) == int(lens.sum()) == res["numbered_bytes"] > res["kept_bytes"] > 0


def test_an_empty_batch_still_writes_the_result(gpu_ctx):
    for cap in (0, 5):
        _, _, _, res, _ = run_case(gpu_ctx, np.zeros(0, np.uint32), cap, None, 3, 0, 1, where="empty")
        assert res == dict(abi.FlowSeqResult().as_dict())


def test_continuity_across_calls(gpu_ctx):
    """The property the feature exists for: the largest batch fed as successive calls of 64, 1,000 and
    16,384 packets against one table gives the concatenation of the whole-batch call's outputs and its
    table. The sequence of calls is made twice, each time from a zero table."""
    n = BIG
    ids, cap = pattern("skewed")
    bits = np.random.default_rng(9).integers(0, 4, n) != 0
    mp, mb, flags = 5, 4000, qr.KEEP_UNKEYED
    ids = ids.copy()
    ids[::97] = 0xFFFFFFFE
    wseq, woff, wout, wres, wtable = run_case(gpu_ctx, ids, cap, fr.pack_bits(bits), mp, mb, flags, where="whole")
    src = crafted_source(gpu_ctx, n, "packed")
    d_ids = upload(gpu_ctx, ids)
    try:
        for _ in range(2):
            tab = Guarded(gpu_ctx, 16 * cap)
            try:
                abi._check(abi.lib().bt_memset_d(gpu_ctx.h, tab.ptr, 0, 16 * cap))
                seqs, offs, keep, lo = [], [], [], 0
                total = dict.fromkeys(("selected", "numbered", "unkeyed", "kept", "numbered_bytes", "kept_bytes", "new_flows"), 0)
                for cnt in itertools.cycle((64, 1000, 16384)):
                    cnt = min(cnt, n - lo)
                    batch = abi.Batch(src.d_data.ptr, src.d_desc.ptr + 8 * lo, 0, cnt, src.batch.bytes, abi.DESC_PACKED, 0)
                    seq, off, out, res = device_once(gpu_ctx, batch, cnt, d_ids.ptr + 4 * lo, fr.pack_bits(bits[lo:lo + cnt]), cap,
                                                     tab.ptr, mp, mb, flags, SEQ | OFF | SEL)
                    seqs.append(seq)
                    offs.append(off)
                    keep.append(fr.select_bits(out, cnt).astype(bool))
                    for k in total:
                        total[k] += res[k]
                    lo += cnt
                    if lo == n:
                        break
                assert (np.concatenate(seqs) == wseq).all() and (np.concatenate(offs) == woff).all()
                assert (fr.pack_bits(np.concatenate(keep)) == wout).all()
                assert tab.read().tobytes() == wtable.tobytes()
                assert total == {k: wres[k] for k in total}
            finally:
                tab.free()
    finally:
        src.free()
        d_ids.free()


@pytest.mark.parametrize("name", ["http", "edge"])
def test_the_table_goes_through_a_device_expire_by_the_side_move(gpu_ctx, name):
    """The GPU twin of test_flowseq.py's host case: a device tracker numbers two batches; the sequence table
    follows a device expire by bt_flow_track_side_move_device with rec_bytes = 16, and a third batch goes on
    where its flows were. Flow numbers and the remap come from flowtrack_ref, positions from flowseq_ref;
    every call is enqueued on one stream and waited for once."""
    ctx = gpu_ctx
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    half = n0 // 2
    desc = g["desc"].astype(np.uint64)
    lens = (desc >> np.uint64(48)).astype(np.int64)
    keys = golden_keys(name)
    parts = [(slice(0, half), 100), (slice(half, n0), 5000), (slice(half, n0), 5001)]
    ref, want = fkr.Tracker(n0, 0), np.zeros(n0, qr.SEQ_REC)
    lay = abi.flow_track_layout(n0, 0)
    need = max([abi.flow_track_scratch_bytes(n0), abi.flow_seq_scratch_bytes(n0, n0), abi.flow_track_expire_scratch_bytes(n0),
                abi.flow_track_side_move_scratch_bytes(n0, 16)])
    state, table, scratch = Guarded(ctx, lay["total"]), Guarded(ctx, 16 * n0), Guarded(ctx, need)
    exp = {"expired": Guarded(ctx, 104 * n0), "side": Guarded(ctx, 16 * n0), "remap": Guarded(ctx, 4 * n0), "res": Guarded(ctx, 32)}
    srcs, outs, wants = [], [], []
    st = ctx.stream_create()
    started = False
    try:
        abi._check(abi.lib().bt_memset_d(ctx.h, table.ptr, 0, 16 * n0))
        for k, (sl, ts) in enumerate(parts):
            if k == 2:   # the restatement's expire between the second and the third batch
                before = want.copy()
                e = ref.expire(5000, 1000, n0)
                r = e["result"]
                assert r["n_expired"] > 0 and r["n_flows"] > 0
                gone = before[:r["n_flows_before"]][e["remap"] == fkr.EXPIRED]
                want[:] = 0
                stay = e["remap"] != fkr.EXPIRED
                want[e["remap"][stay]] = before[:r["n_flows_before"]][stay]
            n = sl.stop - sl.start
            ids = ref.update(keys[0][sl], keys[1][sl], keys[2][sl], lens[sl], None, None, ts)["flow_id"]
            wants.append(qr.number(want, ids, lens[sl], None, 3) + (ids,))
            srcs.append(Source(ctx, name, n, "packed", desc=desc[sl]))
            outs.append({"ids": Guarded(ctx, 4 * n), "seq": Guarded(ctx, 4 * n), "off": Guarded(ctx, 8 * n), "words": Guarded(ctx, 8 * ((n + 63) // 64)),
                         "track": Guarded(ctx, 64), "res": Guarded(ctx, 64)})
        ctx.synchronize()
        ctx.flow_track_init(state.ptr, lay["total"], n0, 0, 0, stream=st)
        started = True
        for k, (src, o, (sl, ts)) in enumerate(zip(srcs, outs, parts)):
            if k == 2:
                ctx.flow_track_expire(state.ptr, 5000, 1000, scratch.ptr, need, exp["res"].ptr, expired=exp["expired"].ptr, expired_cap=n0,
                                      remap=exp["remap"].ptr, stream=st)
                ctx.flow_track_side_move(table.ptr, 16, n0, exp["remap"].ptr, exp["res"].ptr, scratch.ptr, need, expired_side=exp["side"].ptr,
                                         expired_cap=n0, stream=st)
            ctx.flow_track_update(state.ptr, src.batch, scratch.ptr, need, o["track"].ptr, batch_ts=ts, flow_id=o["ids"].ptr, stream=st)
            ctx.flow_seq(src.batch, o["ids"].ptr, None, table.ptr, n0, scratch.ptr, need, o["res"].ptr, max_packets=3, seq=o["seq"].ptr,
                         byte_off=o["off"].ptr, out_select=o["words"].ptr, stream=st)
        ctx.stream_synchronize(st)
        ctx.synchronize()
        scratch.read()   # its guards
        for k, (o, (wseq, woff, wout, wres, ids)) in enumerate(zip(outs, wants)):
            assert (o["ids"].read(np.uint32) == ids).all(), f"batch {k}: flow_id"
            assert abi.FlowSeqResult.from_bytes(o["res"].read()).as_dict() == wres, f"batch {k}: result"
            assert (o["seq"].read(np.uint32) == wseq).all() and (o["off"].read(np.uint64) == woff).all(), f"batch {k}: seq / byte_off"
            assert (o["words"].read(np.uint64) == wout).all(), f"batch {k}: out_select"
        res = abi.FlowTrackExpireResult.from_bytes(exp["res"].read()).as_dict()
        assert res == r and (exp["remap"].read(np.uint32)[:r["n_flows_before"]] == e["remap"]).all()
        side = exp["side"].read()
        assert side[:16 * r["n_expired"]].tobytes() == gone.tobytes() and (side[16 * r["n_expired"]:] == POISON).all(), "the expired flows' records"
        assert exp["expired"].read()[:104 * r["n_expired"]].tobytes() == e["expired"].tobytes()
        assert table.read().tobytes() == want.tobytes(), "the table after the third batch"
        keyed = wants[2][4] < n0
        assert wants[2][3]["new_flows"] == 0 and (wants[2][0][keyed] >= 1).all()   # every flow of the second half survived with its count
    finally:
        if started:
            abi.Context.flow_track_forget(state.ptr)
        ctx.stream_destroy(st)
        for b in [state, table, scratch, *exp.values(), *srcs] + [x for o in outs for x in o.values()]:
            b.free()
