"""GPU: the reassembled TCP stream bytes exported on the device (bt_flow_follow_device,
beatrice_amd/csrc/bt_flowfollow.hip between the stages of bt_flowreasm.hip). The kernels take flow_id and off
directly: the ids are crafted and the offsets come from bt_flow_tcpseq_host on the same frames. Every device
call is compared byte for byte with the host form and with the restatement in flowfollow_ref.py: the bytes,
the runs, place, both results, hit, rest and the table. Every output, the table and the scratch sit in
poisoned buffers between two 256-byte guards; the scratch is filled with 0xA5 first and is exactly
bt_flow_follow_scratch_bytes long; every call is made twice from the same starting table and the two runs
must be byte-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowfollow_ref as fr  # noqa: E402
import flowreasm_cases as rc  # noqa: E402
import flowreasm_ref as rr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowfollow import follow_result_of  # noqa: E402
from test_flowreasm import result_of, select_of  # noqa: E402
from test_flowstream import lay_out, words_of  # noqa: E402
from test_gpu_flowstream import Frames, Pattern, upload  # noqa: E402
from test_gpu_flowtab import FORMATS, POISON, Guarded, Source  # noqa: E402

pytestmark = pytest.mark.gpu

BIDIR = 2
UNIT, CHUNK = 2048, 16384   # kFsUnit, kFsChunk
REC = 128


class CutFrames:
    """Packed frames whose buffer ends `cut` bytes early: the last frame's descriptor runs past the end, and the
    bytes it does not hold read as zero."""

    def __init__(self, ctx, frames, cut):
        data, self.desc = lay_out(frames)
        end = int(self.desc[-1] & np.uint64((1 << 48) - 1)) + len(frames[-1])   # lay_out may pad behind the last frame
        self.data = data[:end - cut].copy()
        self.seen = [bytes(f) for f in frames[:-1]] + [bytes(frames[-1][:len(frames[-1]) - cut]) + bytes(cut)]
        self.src = Source(ctx, "c3", len(frames), "packed", data=self.data, desc=self.desc)
        self.batch = self.src.batch

    def free(self):
        self.src.free()


def device_once(ctx, pat, batch, n, d_ids, d_off, sel, flags, cap, tab_ptr, ocap, rcap, alias=None, stream=None, reasm=False):
    """One bt_flow_follow_device (or, with reasm, bt_flow_reasm_device) into guarded outputs and a guarded scratch
    full of 0xA5. Returns (hit, rest, result, bytes, runs, place, follow result)."""
    nw = (n + 63) // 64
    need = abi.flow_reasm_scratch_bytes(n, cap) if reasm else abi.flow_follow_scratch_bytes(n, cap)
    hit, rest = Guarded(ctx, 8 * nw), Guarded(ctx, 8 * nw)
    res, fres, scratch = Guarded(ctx, 64), Guarded(ctx, 32), Guarded(ctx, need)
    out, runs, place = Guarded(ctx, ocap), Guarded(ctx, 32 * rcap), Guarded(ctx, 8 * n)
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
        common = (batch, d_ids, sel_ptr, d_off, flags, pat.blob if pat else None, pat.dev if pat else None, tab_ptr if cap else None, cap,
                  scratch.ptr if n else None, need, res.ptr)
        if reasm:
            ctx.flow_reasm(*common, hit=hit.ptr if nw else None, rest=rest.ptr if nw else None, stream=stream)
        else:
            ctx.flow_follow(*common, fres.ptr, out_bytes=out.ptr if ocap else None, cap=ocap, runs=runs.ptr if rcap else None, run_cap=rcap,
                            place=place.ptr if n else None, hit=hit.ptr if nw else None, rest=rest.ptr if nw else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        scratch.read()   # its guards
        return (hit.read(np.uint64), rest.read(np.uint64), abi.FlowReasmResult.from_bytes(res.read()).as_dict(), out.read(),
                runs.read().view(abi.FlowFollowRun), place.read(np.uint64), None if reasm else abi.FlowFollowResult.from_bytes(fres.read()).as_dict())
    finally:
        for g in (hit, rest, res, fres, scratch, out, runs, place, d_sel):
            if g is not None:
                g.free()


def run_case(ctx, pat, calls, cap, flags=BIDIR, fmt="packed", alias=None, stream=None, caps=None, where="", cut=0, against_reasm=False):
    """calls: [rows]. Per call: the offsets by bt_flow_tcpseq_host, the restatement, the device call twice from the
    same table, the host form; the tables carry on. caps: None (frames->bytes and n: always enough) or a function
    (total, n_runs) -> (cap, run_cap). Returns [(bytes, runs, result, follow result, the table after)]."""
    blob = pat.blob if pat else None
    model = fr.Follow(cap, blob, flags)
    table = np.zeros(cap, rr.REC)
    seq_tab = np.zeros(cap, abi.FlowTcpseqRec)
    got = []
    for k, rows in enumerate(calls):
        at = f"{where} call {k}"
        n, nw = len(rows), (len(rows) + 63) // 64
        ids = np.ascontiguousarray([r.flow for r in rows], np.uint32)
        src = CutFrames(ctx, [r.frame for r in rows], cut) if cut else Frames(ctx, [r.frame for r in rows], fmt)
        sel = select_of(rows)
        if alias and sel is None:
            sel = words_of([True] * n)
        off = np.full(n, 7, np.int64)
        abi.flow_tcpseq_host(src.data, src.desc, ids, sel, flags, seq_tab, off=off)
        d_ids, d_off = upload(ctx, ids), upload(ctx, off)
        want_hit, want_rest, want_res, wbytes, wruns, wplace, wfres = model.follow(src.seen, ids, off, sel)
        ocap, rcap = (len(src.data), n) if caps is None else caps(wfres["total"], wfres["n_runs"])
        wfres = dict(wfres, written=min(wfres["total"], ocap), runs_written=min(wfres["n_runs"], rcap))
        w, kr = wfres["written"], wfres["runs_written"]
        wtab = model.table
        runs_ = []
        try:
            for _ in range(2):
                tab = Guarded(ctx, REC * cap)
                try:
                    if cap:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, table.ctypes.data, REC * cap))
                    hit, rest, res, out, runs, place, fres = device_once(ctx, pat, src.batch, n, d_ids, d_off, sel, flags, cap, tab.ptr, ocap, rcap,
                                                                         alias, stream)
                    after = tab.read()
                finally:
                    tab.free()
                assert res["reserved0"] == 0 and res["reserved1"] == 0
                assert result_of(res) == want_res, f"{at}: result {result_of(res)} != {want_res}"
                assert follow_result_of(fres) == wfres, f"{at}: follow result {fres} != {wfres}"
                assert (hit == want_hit).all() and (rest == want_rest).all(), f"{at}: hit / rest"
                bad = np.nonzero((after.view(np.uint64).reshape(-1, 16) != wtab.view(np.uint64).reshape(-1, 16)).any(axis=1))[0]
                assert len(bad) == 0, f"{at}: table differs at flows {bad[:8]}: {after.view(rr.REC)[bad[:2]]} != {wtab[bad[:2]]}"
                bad = np.nonzero(out[:w] != np.frombuffer(wbytes[:w], np.uint8))[0]
                assert len(bad) == 0, f"{at}: bytes differ at {bad[:8]} of {w}: {out[bad[:8]]} != {np.frombuffer(wbytes, np.uint8)[bad[:8]]}"
                assert (out[w:] == POISON).all(), f"{at}: bytes written at or past `written`"
                assert runs[:kr].tobytes() == wruns[:kr].tobytes(), f"{at}: runs {runs[:kr][:4]} != {wruns[:kr][:4]}"
                assert (runs[kr:].view(np.uint8) == POISON).all(), f"{at}: runs written past runs_written"
                bad = np.nonzero(place != wplace)[0]
                assert len(bad) == 0, f"{at}: place differs at {bad[:8]}"
                runs_.append((hit.tobytes(), rest.tobytes(), after.tobytes(), out.tobytes(), runs.tobytes(), place.tobytes()))
            assert runs_[0] == runs_[1], f"{at}: two runs differ"
            if n:   # the host form, byte for byte
                host = table.copy().view(abi.FlowReasmRec)
                hhit, hrest = np.full(nw, 0xDEAD, np.uint64), np.full(nw, 0xDEAD, np.uint64)
                hout, hruns = np.full(ocap, POISON, np.uint8), np.frombuffer(bytes([POISON]) * (32 * rcap), abi.FlowFollowRun).copy()
                hplace = np.zeros(n, np.uint64)
                hres, hfres = abi.flow_follow_host(src.data, src.desc, ids, sel, off, flags, blob, host, out_bytes=hout, runs=hruns, place=hplace,
                                                   hit=hhit, rest=hrest)
                assert result_of(hres) == want_res and follow_result_of(hfres) == wfres, f"{at}: the host form's results"
                assert (hhit.tobytes(), hrest.tobytes(), host.tobytes(), hout.tobytes(), hruns.tobytes(), hplace.tobytes()) == runs_[0], f"{at}: the host form"
            if against_reasm and n:   # bt_flow_reasm_device on a copy of the same starting table
                tab = Guarded(ctx, REC * cap)
                try:
                    abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tab.ptr, table.ctypes.data, REC * cap))
                    rhit, rrest, rres, _, _, _, _ = device_once(ctx, pat, src.batch, n, d_ids, d_off, sel, flags, cap, tab.ptr, 0, 0, None, stream, reasm=True)
                    assert (rhit.tobytes(), rrest.tobytes(), tab.read().tobytes()) == runs_[0][:3] and rres == res, f"{at}: bt_flow_reasm_device"
                finally:
                    tab.free()
        finally:
            for x in (src, d_ids, d_off):
                x.free()
        table = wtab.copy()
        got.append((wbytes, wruns, want_res, wfres, wtab))
    return got


@pytest.fixture
def hello(gpu_ctx):
    pat = Pattern(gpu_ctx, rc.PATTERN)
    yield pat
    pat.free()


def test_the_named_cases_and_the_reassembly_call_from_the_same_table(gpu_ctx, hello):
    calls, cap, _ = rc.crafted()
    got = run_case(gpu_ctx, hello, calls, cap, where="crafted", against_reasm=True)
    assert got[0][3]["n_runs"] > 15 and sum(g[2]["hit_packets"] for g in got) > 5
    run_case(gpu_ctx, hello, calls, cap, 0, where="crafted, one direction")
    calls, cap = rc.long_pattern()
    pat = Pattern(gpu_ctx, rc.LONG)
    try:
        run_case(gpu_ctx, pat, calls, cap, where="long", against_reasm=True)
    finally:
        pat.free()


@pytest.mark.parametrize("fmt", FORMATS)
def test_clean_and_disturbed_captures_in_every_descriptor_format_on_a_stream_of_its_own(gpu_ctx, fmt):
    pat = Pattern(gpu_ctx, "GET|POST")
    st = gpu_ctx.stream_create()
    try:
        for seed in (2, 5):
            calls, truth = rc.random_calls(seed, nflows=3, nbytes=500 + 97 * seed, ncalls=1 + seed % 3, clean=True)
            got = run_case(gpu_ctx, pat, calls, 3, fmt=fmt, stream=st, alias="hit" if seed == 2 else None, where=f"clean {seed} {fmt}")
            streams = {}
            for wbytes, wruns, _, _, _ in got:
                for u in wruns:
                    assert not u["flags"] & fr.HOLE
                    key = (int(u["flow"]), int(u["flags"]) & 1)
                    streams[key] = streams.get(key, b"") + wbytes[int(u["at"]):int(u["at"] + u["len"])]
            assert streams == truth
        for seed in (1, 4):
            calls, _ = rc.random_calls(100 + seed, nflows=4, nbytes=700, ncalls=3, clean=False)
            got = run_case(gpu_ctx, pat, calls, 4, fmt=fmt, stream=st, alias="rest" if seed == 1 else None, where=f"disturbed {seed} {fmt}")
            assert sum(int(((g[1]["flags"] & fr.HOLE) != 0).sum()) for g in got) >= 2 and sum(g[2]["late_packets"] for g in got) > 0
    finally:
        gpu_ctx.stream_destroy(st)
        pat.free()


def seam_rows():
    """One flow whose segments have the lengths 1, 15, 16, 17, 31, 33, 64 and 1460, repeated in rotating order, each
    starting 0 to 3 bytes inside the one before (those bytes are trimmed), so that the destination offset mod 16
    and the source offset mod 16 of the first delivered byte each take all 16 values; and a whole duplicate (length
    0 after trimming) in the middle of the first tile. Returns (rows, [(the bytes into the frame of the first
    delivered byte, the delivered length) per row])."""
    c = rc.Conn(0, rc.M32 - 5000, 9, sp=47000)
    stream = np.random.default_rng(7).integers(1, 255, 40000, dtype=np.uint8).tobytes()
    lens = [1, 15, 16, 17, 31, 33, 64, 1460]
    rows, facts, at, prev = [], [], 0, 1
    for k in range(18):
        for j in range(8):
            ln = lens[(j + k) % 8]
            ov = min((k + j) % 4, prev - 1, ln - 1)
            rows.append(rc.seg(c, 0, at - ov, stream[at - ov:at - ov + ln]))
            facts.append((len(rows[-1].frame) - ln + ov, ln - ov))
            at += ln - ov
            prev = ln
            if len(rows) == 30:
                rows.append(rows[-3].again_data())
                facts.append((0, 0))
    return rows, facts, stream[:at]


def test_the_copy_at_every_alignment_of_source_and_destination(gpu_ctx):
    rows, facts, stream = seam_rows()
    data, desc = lay_out([r.frame for r in rows])
    src_mod = {(int(d) & ((1 << 48) - 1)) + f[0] for d, f in zip(desc, facts) if f[1]}
    dst_mod, at = set(), 0
    for _, ln in facts:
        if ln:
            dst_mod.add(at % 16)
        at += ln
    assert {x % 16 for x in src_mod} == set(range(16)) and dst_mod == set(range(16)) and at == len(stream)
    got = run_case(gpu_ctx, None, [rows], 1, where="seams")
    assert got[0][0] == stream and got[0][3]["n_runs"] == 1 and got[0][2]["dup_packets"] == 1
    # a cap that ends inside a 16-B line and inside a segment
    run_case(gpu_ctx, None, [rows], 1, caps=lambda t, r: (1 + 15 + 16 + 17 + 31 + 33 + 64 + 1000 + 7, r), where="seams, cap")
    run_case(gpu_ctx, None, [rows], 1, caps=lambda t, r: (5, 0), where="seams, 5 bytes and no run")
    run_case(gpu_ctx, None, [rows], 1, caps=lambda t, r: (0, 1), where="seams, a size query with one run")
    # the last frame's descriptor runs 700 bytes past the buffer's end: zeros
    big = [i for i, r in enumerate(rows[:64]) if len(r.data) == 1460][-1]
    rows = rows[:big + 1]
    got = run_case(gpu_ctx, None, [rows], 1, where="past the end", cut=700)
    assert got[0][0][-700:] == bytes(700) and got[0][0][-701] != 0


def tiny_rows(n, seed, nconn=3):
    """n packets of nconn connections, both directions round robin: one-to-three-byte segments, here and there one
    dropped (a hole), swapped with its neighbour or sent twice."""
    rng = np.random.default_rng(seed)
    conns = [rc.Conn(f, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), sp=48000 + f) for f in range(nconn)]
    at = [[0, 0] for _ in conns]
    rows = []
    while len(rows) < n:
        k = len(rows) % (2 * nconn)
        f, d = k >> 1, k & 1
        ln = int(rng.integers(1, 4))
        op = int(rng.integers(0, 40))
        if op == 0:
            at[f][d] += 2   # dropped bytes
        rows.append(rc.seg(conns[f], d, at[f][d], rng.integers(65, 91, ln, dtype=np.uint8).tobytes()))
        at[f][d] += ln
        if op == 1 and len(rows) < n:
            rows.append(rows[-1].again_data())
        if op == 2 and len(rows) > 2 * nconn:
            rows[-1], rows[-1 - 2 * nconn] = rows[-1 - 2 * nconn], rows[-1]
    return rows[:n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 16384, 16385])
def test_sizes_at_the_edges_of_tile_unit_and_chunk(gpu_ctx, n):
    got = run_case(gpu_ctx, None, [tiny_rows(n, n)], 3, where=f"n={n}")
    assert got[0][2]["n"] == n and got[0][3]["total"] >= n * 9 // 10 and got[0][3]["n_runs"] >= min(n, 6)


def test_one_run_across_a_unit_and_a_chunk_of_the_sorted_list(gpu_ctx, hello):
    """One stream of CHUNK + 116 tiny segments in reverse arrival behind a short one: its single run starts in the first
    unit and ends in the second chunk."""
    a = [rc.seg(rc.Conn(0, 77, 9, sp=41000), 0, k, b"ab"[k % 2:k % 2 + 1]) for k in range(40)]
    c = rc.Conn(1, rc.M32 - 100, 9, sp=41001)
    b = [rc.seg(c, 0, 2 * k, bytes([65 + k % 26, 97 + k % 26])) for k in range(CHUNK + 116)][::-1]
    got = run_case(gpu_ctx, hello, [a + b], 2, where="unit and chunk")
    assert got[0][3]["n_runs"] == 2 and int(got[0][1][1]["len"]) == 2 * (CHUNK + 116)


def test_sixty_four_directions_in_one_tile(gpu_ctx):
    """32 connections, both directions, one segment each: a run head in every lane; then the same again: 64 runs that continue."""
    conns = [rc.Conn(f, 1000 * f, 7 * f, sp=49000 + f) for f in range(32)]
    first = [rc.seg(conns[k >> 1], k & 1, 0, bytes([65 + k % 26]) * (1 + k % 5)) for k in range(64)]
    second = [rc.seg(conns[k >> 1], k & 1, 1 + k % 5, bytes([97 + k % 26]) * (1 + k % 3)) for k in range(64)][::-1]
    got = run_case(gpu_ctx, None, [first, second], 32, where="64 directions")
    assert got[0][3]["n_runs"] == 64 and ((got[0][1]["flags"] & 6) == fr.NEW).all()
    assert got[1][3]["n_runs"] == 64 and ((got[1][1]["flags"] & 6) == 0).all()


def test_a_batch_without_tcp(gpu_ctx, hello):
    rows = [rc.other(rc.tcp(1, payload=b"HELLO", proto=17, sp=40000 + k), k % 3) for k in range(70)]
    got = run_case(gpu_ctx, hello, [rows], 3, where="no tcp")
    assert got[0][3] == {"total": 0, "written": 0, "n_runs": 0, "runs_written": 0} and got[0][2]["selected"] == 70
    got = run_case(gpu_ctx, hello, [[]], 3, where="empty")
    assert got[0][3]["total"] == 0 and got[0][2]["n"] == 0


def test_three_consecutive_calls_on_one_table(gpu_ctx, hello):
    """The first run of call k + 1 continues at call k's next with neither flag; a dropped segment gives a hole run whose
    distance from the end before it is what hole_bytes grew by."""
    c = rc.Conn(0, rc.M32 - 20, 9, sp=46000)
    s = bytes(range(48, 48 + 60))
    calls = [[rc.seg(c, 0, 10, s[10:20]), rc.seg(c, 0, 0, s[0:10])],
             [rc.seg(c, 0, 20, s[20:25]), rc.seg(c, 0, 32, s[32:40])],          # 7 bytes dropped
             [rc.seg(c, 0, 40, s[40:60])]]
    got = run_case(gpu_ctx, hello, calls, 1, where="three calls")
    r0, r1, r2 = (g[1] for g in got)
    assert len(r0) == 1 and int(r0[0]["flags"]) == fr.NEW and got[0][0] == s[0:20]
    nxt = [int(g[4][0]["d"][0]["next"]) for g in got]
    assert len(r1) == 2 and int(r1[0]["flags"]) == 0 and int(r1[0]["pos"]) == nxt[0] and int(r1[1]["flags"]) == fr.HOLE
    grew = int(got[1][4][0]["d"][0]["hole_bytes"]) - int(got[0][4][0]["d"][0]["hole_bytes"])
    assert int(r1[1]["pos"]) - (int(r1[0]["pos"]) + int(r1[0]["len"])) == grew == 7
    assert len(r2) == 1 and int(r2[0]["flags"]) == 0 and int(r2[0]["pos"]) == nxt[1] and got[2][0] == s[40:60]


def test_the_capacities_on_the_device(gpu_ctx, hello):
    calls, _ = rc.random_calls(104, nflows=4, nbytes=700, ncalls=2, clean=False)
    for caps in (lambda t, r: (0, 0), lambda t, r: (1, 1), lambda t, r: (t - 1, r - 1), lambda t, r: (t, r)):
        run_case(gpu_ctx, hello, calls, 4, caps=caps, where="caps")


def test_without_a_pattern_on_the_device(gpu_ctx, hello):
    calls, cap, _ = rc.crafted()
    with_pat = run_case(gpu_ctx, hello, calls, cap, where="with")
    plain = run_case(gpu_ctx, None, calls, cap, alias="hit", where="plain")
    for a, b in zip(with_pat, plain):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[3] == b[3] and b[2]["hit_packets"] == 0
        assert (b[4]["d"]["d"] == 0).all() and (a[4]["d"]["next"] == b[4]["d"]["next"]).all()


def test_a_scratch_one_byte_short_is_refused(gpu_ctx, hello):
    ctx = gpu_ctx
    rows = tiny_rows(100, 4)
    src = Frames(ctx, [r.frame for r in rows], "packed")
    bufs = [upload(ctx, np.zeros(100, np.uint32)), upload(ctx, np.zeros(100, np.int64)), Guarded(ctx, REC), Guarded(ctx, 64), Guarded(ctx, 32)]
    need = abi.flow_follow_scratch_bytes(100, 1)
    scratch = Guarded(ctx, need)
    try:
        with pytest.raises(abi.BtError, match="scratch_bytes"):
            ctx.flow_follow(src.batch, bufs[0], None, bufs[1], BIDIR, hello.blob, hello.dev, bufs[2].ptr, 1, scratch.ptr, need - 1, bufs[3].ptr,
                            bufs[4].ptr)
    finally:
        for x in [src, scratch] + bufs:
            x.free()
