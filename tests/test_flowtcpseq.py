"""CPU: TCP segments classified per flow and direction on the host (bt_flow_tcpseq_host) against the
restatement in flowtcpseq_ref.py (Python integers, a dict per direction) and against the class the case
generator recorded from the true 64-bit offsets; the entry points' refusals (decided before the context,
so with a null one), `out_select` in place of `select`, and the record through the side move."""
import ctypes
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
from test_flowstream import lay_out, words_of  # noqa: E402

BIDIR = 2
BT_E_INVALID_ARGUMENT = 1


def host_against_ref(batches, cap, flags, start=None, truth=True, where=""):
    """Every batch ((frames, ids, select bits, rows)) through the host form and through the restatement from the
    same table; with `truth` both against the generator's classes and offsets. Returns the restatement and
    the per-batch (cls, off, out_select, result)."""
    model = tr.Space(cap, flags, start)
    table = np.zeros(cap, abi.FlowTcpseqRec) if start is None else start.copy().view(abi.FlowTcpseqRec)
    outs = []
    for k, (frames, ids, bits, rows) in enumerate(batches):
        at = f"{where} batch {k}"
        n = len(frames)
        data, desc = lay_out(frames)
        sel = None if all(bits) else words_of(bits)
        if sel is not None and n % 64:
            sel[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
        want = model.batch(frames, ids, sel)
        cls, off, osel = np.full(n, 0xEE, np.uint8), np.full(n, 12345, np.int64), np.full((n + 63) // 64, 0xDEADBEEF, np.uint64)
        res = abi.flow_tcpseq_host(data, desc, np.array(ids, np.uint32), sel, flags, table, cls=cls, off=off, out_select=osel)
        assert res == want[3], f"{at}: result {res} != {want[3]}"
        bad = np.nonzero(cls != want[0])[0]
        assert len(bad) == 0, f"{at}: class differs at packets {bad[:8]}: {cls[bad[:8]]} != {want[0][bad[:8]]}"
        assert (off == want[1]).all() and (osel == want[2]).all(), f"{at}: off / out_select"
        assert table.tobytes() == model.table.tobytes(), f"{at}: table"
        if truth and rows is not None:
            got = [(int(c), None if int(o) == tr.OFF_NONE else int(o)) for c, o in zip(cls, off)]
            assert got == [(r.want, r.u) for r in rows], f"{at}: the generator's truth"
        outs.append((cls, off, osel, res))
    return model, outs


def split(rows, k):
    for r in rows:
        r.batch = 0
    for r in rows[k:]:
        r.batch = 1
    return tc.batches_of(rows)


def test_the_named_cases_against_the_restatement_and_the_truth():
    rows, cap = tc.crafted()
    model, outs = host_against_ref(tc.batches_of(rows), cap, BIDIR, where="crafted")
    total = {k: sum(o[3][k] for o in outs) for k in ("first", "in_order", "gap", "old", "overlap", "unkeyed", "bad_ids")}
    assert total["unkeyed"] == 4 and total["bad_ids"] == 2 and min(total.values()) > 0
    # without directions both sides of a connection share one sequence space: no truth, the restatement alone
    host_against_ref(tc.batches_of(rows), cap, 0, truth=False, where="crafted, one direction")


def test_the_same_packets_split_at_every_position_into_two_calls():
    rows, cap = tc.crafted()
    tc.truth(rows)
    whole = None
    for k in range(len(rows) + 1):
        model, outs = host_against_ref(split(rows, k), cap, BIDIR, where=f"split {k}")
        if whole is None:
            whole = model.table.tobytes()
        assert model.table.tobytes() == whole, f"split {k}: the table depends on the split"


@pytest.mark.parametrize("seed", range(6))
def test_random_conversations(seed):
    rows = tc.random_set(seed)
    host_against_ref(tc.batches_of(rows), 4, BIDIR, where=f"seed {seed}")
    cut = len(rows) // 3
    for r in rows[cut:]:
        r.batch = 1
    for r in rows[2 * cut:]:
        r.batch = 2
    host_against_ref(tc.batches_of(rows), 4, BIDIR, where=f"seed {seed} in three calls")


def classes_of(rows, cap=1, flags=BIDIR):
    tc.truth(rows)
    _, outs = host_against_ref(tc.batches_of(rows), cap, flags)
    return [int(c) for c in outs[0][0]], [int(o) for o in outs[0][1]], outs[0][3]


def test_syn_and_fin_each_consume_one_sequence_number():
    c = tc.Conn(0, 1000)
    rows = [c.seg(0, 0, 0, tc.SYN), c.seg(0, 1, 10), c.seg(0, 0, 0, tc.SYN), c.seg(0, 11, 0, tc.FIN | tc.ACK), c.seg(0, 12, 5),
            c.seg(0, 11, 0, tc.FIN | tc.ACK), c.seg(0, 17, 3, tc.SYN | tc.FIN)]
    cls, off, res = classes_of(rows)
    assert cls == [tc.FIRST, tc.IN_ORDER, tc.OLD, tc.IN_ORDER, tc.IN_ORDER, tc.OLD, tc.IN_ORDER]
    assert off == [0, 1, 0, 11, 12, 11, 17] and res["seq_bytes"] == 1 + 10 + 1 + 1 + 5 + 1 + 5 and res["old_bytes"] == 2


def test_what_does_not_participate_leaves_the_record_untouched():
    c = tc.Conn(0, 77)
    quiet = [c.ack(0, 5), c.ack(0, 5, tc.RST), c.ack(0, 5, tc.RST | tc.ACK), tc.Row(tc.tcp(82, 10, proto=17), 0),
             tc.Row(tc.tcp(82, 10, frag=0x2000), 0), tc.Row(tc.tcp(82, 10, frag=1), 0), tc.Row(tc.tcp(82, 10)[:14 + 20 + 19], 0),
             tc.Row(tc.tcp(82, 10, proto=1), 0)]
    table = np.zeros(1, abi.FlowTcpseqRec)
    data, desc = lay_out([r.frame for r in quiet])
    cls, off = np.full(len(quiet), 9, np.uint8), np.zeros(len(quiet), np.int64)
    res = abi.flow_tcpseq_host(data, desc, np.zeros(len(quiet), np.uint32), None, BIDIR, table, cls=cls, off=off)
    assert not cls.any() and (off == abi.TCPSEQ_OFF_NONE).all() and not table.view(np.uint64).any()
    assert res["selected"] == len(quiet) and res["seq_packets"] == 0
    rows = [c.seg(0, 0, 5)] + quiet + [c.seg(0, 5, 5)]
    cls, off, res = classes_of(rows)
    assert cls == [tc.FIRST] + [tc.NONE] * len(quiet) + [tc.IN_ORDER] and res["seq_packets"] == 2


def test_a_step_of_two_to_the_31_is_taken_as_minus():
    c = tc.Conn(0, 5)
    rows = [c.seg(0, 0, 10), c.seg(0, -(1 << 31), 10)]
    cls, off, res = classes_of(rows)
    assert cls == [tc.FIRST, tc.OLD] and off == [0, -(1 << 31)]
    rows = [c.seg(0, 0, 10), c.seg(0, (1 << 31) - 1, 10)]
    cls, off, res = classes_of(rows)
    assert cls == [tc.FIRST, tc.GAP] and off == [0, (1 << 31) - 1] and res["gap_bytes"] == (1 << 31) - 11


def test_a_long_flow_follows_the_wrap_many_times():
    """Steps of 2^30 bytes (headers only: the frames are snapped): twelve of them wrap three times, and the
    unwrapped offsets keep growing."""
    c = tc.Conn(0, tc.M32 - 10)
    rows = [c.seg(0, 0, 100, snap=60)] + [c.seg(0, k << 30, 100, snap=60) for k in range(1, 13)] + [c.seg(0, 12 << 30, 100, snap=60)]
    cls, off, res = classes_of(rows)
    assert cls == [tc.FIRST] + [tc.GAP] * 12 + [tc.OLD] and off[-2] == 12 << 30 and res["gap_bytes"] == (12 << 30) - 12 * 100


def test_out_select_may_be_select():
    rows = tc.random_set(3, nflows=6, nseg=20)
    frames, ids = [r.frame for r in rows], np.array([r.flow for r in rows], np.uint32)
    data, desc = lay_out(frames)
    sel = words_of([i % 5 != 2 for i in range(len(rows))])
    apart, t1 = np.zeros_like(sel), np.zeros(6, abi.FlowTcpseqRec)
    r1 = abi.flow_tcpseq_host(data, desc, ids, sel.copy(), BIDIR, t1, out_select=apart)
    both, t2 = sel.copy(), np.zeros(6, abi.FlowTcpseqRec)
    r2 = abi.flow_tcpseq_host(data, desc, ids, both, BIDIR, t2, out_select=both)
    assert r1 == r2 and (apart == both).all() and t1.tobytes() == t2.tobytes() and r1["old"] > 0
    assert sum(bin(int(w)).count("1") for w in both) == r1["selected"] - r1["old"] and not (both & ~sel).any()
    d = abi.decode_flow_tcpseq(t1[0])
    assert d["have"] == [True, True] and d["seq_packets"][0] == int(t1[0]["d"][0]["seq_packets"]) and d["hi"][0] == int(t1[0]["d"][0]["hi"])


def test_each_output_is_optional():
    rows, cap = tc.crafted()
    frames, ids = [r.frame for r in rows], np.array([r.flow for r in rows], np.uint32)
    data, desc = lay_out(frames)
    tabs = []
    for want in ((), ("cls",), ("off",), ("out_select",)):
        t = np.zeros(cap, abi.FlowTcpseqRec)
        kw = {}
        if "cls" in want:
            kw["cls"] = np.zeros(len(rows), np.uint8)
        if "off" in want:
            kw["off"] = np.zeros(len(rows), np.int64)
        if "out_select" in want:
            kw["out_select"] = np.zeros((len(rows) + 63) // 64, np.uint64)
        tabs.append((abi.flow_tcpseq_host(data, desc, ids, None, BIDIR, t, **kw), t.tobytes()))
    assert all(x == tabs[0] for x in tabs)


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is reported
    by its own reason, the null context last."""
    L = abi.lib()
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 64)()
    res = (ctypes.c_uint64 * 8)()
    words = (ctypes.c_uint64 * 2)()
    offs = (ctypes.c_int64 * 4)()
    klass = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * (1 << 17))()
    ip, tp, rp, wp, op, kp = (ctypes.addressof(x) for x in (ids, table, res, words, offs, klass))
    sp = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_tcpseq_scratch_bytes(2, 4)
    assert 0 < need <= (1 << 17) - 256 and abi.flow_tcpseq_scratch_bytes(0, 0) >= 256

    def said(rc, word):
        msg = L.bt_last_error().decode()
        assert rc == BT_E_INVALID_ARGUMENT and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def out_of(cls=kp, off=op, out_select=wp, result=rp, reserved=(0, 0)):
        return abi.FlowTcpseqOut(cls, off, out_select, result, (ctypes.c_uint64 * 2)(*reserved))

    def dev(word, frames, flow_id=ip, select=wp, flags=0, tab=tp, cap=4, scratch=sp, nbytes=need, out=out_of()):
        said(L.bt_flow_tcpseq_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, select, flags, tab, cap, scratch,
                                     nbytes, ctypes.byref(out) if out is not None else None, None), word)

    dev("bt_flow_tcpseq_device: null context", good())
    dev("null context", good(), select=None, out=out_of(cls=None, off=None, out_select=None), flags=3)
    dev("null frames", None)
    dev("null out", good(), out=None)
    dev("null result", good(), out=out_of(result=None))
    dev("unknown flag", good(), flags=4)
    for k in range(2):
        dev("reserved is not 0", good(), out=out_of(reserved=[int(j == k) for j in range(2)]))
    dev("null flow_id", good(), flow_id=None)
    dev("null table", good(), tab=None)
    dev("flow_id is not 4-byte aligned", good(), flow_id=ip + 2)
    dev("table is not 8-byte aligned", good(), tab=tp + 4)
    dev("select is not 8-byte aligned", good(), select=wp + 4)
    dev("off is not 8-byte aligned", good(), out=out_of(off=op + 4))
    dev("out_select is not 8-byte aligned", good(), out=out_of(out_select=wp + 4))
    dev("result is not 8-byte aligned", good(), out=out_of(result=rp + 4))
    dev("flow_cap above 2^31", good(), cap=(1 << 31) + 1)
    dev("scratch is not 256-byte aligned", good(), scratch=sp + 8)
    for flag in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f = good()
        f.flags = flag
        dev("BT_BATCH_PREFIXES", f)
    f = good()
    f.bytes = 0
    dev("bytes == 0", f)
    dev("null scratch", good(), scratch=None)
    dev("scratch_bytes", good(), nbytes=need - 1)
    f = good()
    f.n = 0
    dev("null context", f, flow_id=None, tab=None, cap=0, scratch=None, nbytes=0)   # an empty batch needs none of them

    def host(word, base=ctypes.addressof(data), d=ctypes.addressof(desc), flow_id=ip, select=wp, flags=0, tab=tp, cap=4, out=out_of()):
        said(L.bt_flow_tcpseq_host(base, 256, d, 2, flow_id, select, flags, tab, cap, ctypes.byref(out) if out is not None else None), word)

    host("bt_flow_tcpseq_host: null base / desc", d=None)
    host("null out", out=None)
    host("null result", out=out_of(result=None))
    host("unknown flag", flags=0x80000000)
    host("reserved is not 0", out=out_of(reserved=(0, 7)))
    host("null flow_id", flow_id=None)
    host("null table", tab=None)
    host("flow_id is not 4-byte aligned", flow_id=ip + 2)
    host("table is not 8-byte aligned", tab=tp + 4)
    host("select is not 8-byte aligned", select=wp + 4)
    host("result is not 8-byte aligned", out=out_of(result=rp + 4))
    host("off is not 8-byte aligned", out=out_of(off=op + 4))
    host("out_select is not 8-byte aligned", out=out_of(out_select=wp + 4))
    host("flow_cap above 2^31", cap=(1 << 31) + 1)
    # nothing was written by any refused call
    assert not any(table) and not any(res) and not any(words) and not any(offs) and not any(klass)


def test_an_empty_batch_writes_the_result():
    table = np.zeros(3, abi.FlowTcpseqRec)
    res = abi.flow_tcpseq_host(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), None, 0, table)
    assert res == dict(n=0, selected=0, seq_packets=0, first=0, in_order=0, gap=0, old=0, overlap=0, unkeyed=0, bad_ids=0, seq_bytes=0,
                       old_bytes=0, gap_bytes=0) and not table.view(np.uint64).any()


def test_the_record_goes_through_the_side_move():
    """bt_flow_track_side_move_host with rec_bytes = 128: the survivors' sequence spaces go on under their
    new numbers, an expired flow's record is handed out and a returning flow starts again with FIRST."""
    cap = 9
    conns = [tc.Conn(f, tc.M32 - 5 * f, 99 + f, sp=43000 + f) for f in range(cap)]
    first = tc.truth([c.seg(d, 0, 10) for c in conns for d in range(2)] + [c.seg(0, 10, 10) for c in conns])
    model, _ = host_against_ref(tc.batches_of(first), cap, BIDIR, where="before")
    remap = np.array([0xFFFFFFFB if f % 3 == 0 else f - f // 3 - 1 for f in range(cap)], np.uint32)
    result = dict(n_flows_before=cap, n_flows=cap - 3, n_idle=3, n_expired=3, status=0)
    want = model.table.copy()
    want_gone = str_.side_move(want, remap, result, 3)
    moved = model.table.copy().view(abi.FlowTcpseqRec)
    gone = abi.flow_track_side_move_host(moved, remap, result, 3)
    assert moved.tobytes() == want.tobytes() and gone.tobytes() == want_gone.tobytes() and int(gone[1]["d"][0]["seq_packets"]) == 2
    live = [f for f in range(cap) if f % 3]
    second = []
    for f in live:
        r = conns[f].seg(0, 15, 10)   # 5 old bytes, 5 new
        r.flow = int(remap[f])
        second.append(r)
    back = conns[0].seg(0, 20, 10)    # flow 0 came back as a new flow
    back.flow = cap - 3
    second.append(back)
    _, outs = host_against_ref([([r.frame for r in second], [r.flow for r in second], [True] * len(second), None)], cap, BIDIR,
                               start=moved.copy(), where="after")
    assert [int(c) for c in outs[0][0]] == [tc.OVERLAP] * len(live) + [tc.FIRST] and outs[0][3]["old_bytes"] == 5 * len(live)


def test_flowtcpseq_host_check_builds_and_passes(tmp_path):
    """tools/flowtcpseq_host_check.cpp: the argument checks and the host form against an oracle that keeps true
    64-bit offsets in a std::map, under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
    program."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowtcpseq_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "beatrice_amd", "csrc"),
                    os.path.join(root, "tools", "flowtcpseq_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
