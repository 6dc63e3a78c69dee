"""GPU: the whole flow chain on the device (bt_flow_track_update_device, the TCP / statistics / mark
updates, bt_flow_seq_device, bt_flow_mark_select_device, both expires, bt_flow_track_side_move_device
for every side table the expire did not carry, top-K and hosts at checkpoints) driven over the
scenarios of session_cases.py and held to session_ref.SessionModel, a model keyed by the flow key that
never sees a flow number. The state, the side tables, one scratch arena (the largest need, reused by
every call) and every output sit in poisoned buffers between two 256-byte guards. A scenario's buffers
are allocated and uploaded first; then every call is enqueued back to back on one stream, checkpoints
as device-to-device copies on the same stream, and waited for once. The same scenario on a second
state and the context's own stream must give the same bytes, and so must the host forms."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import session_cases as sc  # noqa: E402
import session_ref as sm  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_gpu_flowtab import POISON, Guarded  # noqa: E402
from test_session_model import SIDE_DTYPES, run_host  # noqa: E402

pytestmark = pytest.mark.gpu

SIDES = ("tcp", "stat", "mark", "seq")
RESULTS = (("track", abi.FlowTrackResult), ("tcp", abi.FlowTcpResult), ("stat", abi.FlowStatResult), ("mark", abi.FlowMarkResult),
           ("seq_res", abi.FlowSeqResult), ("msel", abi.FlowMarkSelectResult))
_hip = []


def copy_d2d(dst, src, nbytes, stream):
    """hipMemcpyAsync, device to device, on `stream`: from the HIP runtime the extension itself has loaded."""
    if not _hip:
        abi.lib()
        with open("/proc/self/maps") as fh:
            path = next(line.split()[-1] for line in fh if "libamdhip64" in line)
        _hip.append(ctypes.CDLL(path))
        _hip[0].hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        _hip[0].hipMemcpyAsync.restype = ctypes.c_int
    rc = _hip[0].hipMemcpyAsync(dst, src, nbytes, 3, stream)
    assert rc == 0, f"hipMemcpyAsync: {rc}"


def run_device(ctx, name, stream, fmt="packed"):
    """The scenario through the *_device calls, one wait: one observation per operation, in the shape
    session_cases.compare takes. Without a stream of its own (the context's) only the last checkpoint is
    taken, from the live buffers after the wait; the others are None."""
    scn = sc.scenario(name)
    cap, flags, k = scn.flow_cap, scn.flags, scn.k
    lay = abi.flow_track_layout(cap, scn.slots)
    sizes = {t: d.itemsize for t, d in SIDE_DTYPES.items()}
    batches = [o for o in scn.ops if o["op"] == "batch"]
    arena_bytes = max([abi.flow_track_scratch_bytes(len(o["frames"])) for o in batches]
                      + [abi.flow_seq_scratch_bytes(len(o["frames"]), cap) for o in batches]
                      + [abi.flow_track_expire_scratch_bytes(cap), abi.flow_track_expire_tcp_scratch_bytes(cap),
                         abi.flow_track_top_scratch_bytes(cap, k), abi.flow_track_hosts_scratch_bytes(cap, 0)]
                      + [abi.flow_track_side_move_scratch_bytes(cap, s) for s in sizes.values()])
    owned, calls, readers = [], [], []
    rng = np.random.default_rng(5)

    def guarded(size):
        g = Guarded(ctx, size)
        owned.append(g)
        return g

    def upload(arr):
        d = ctx.alloc(max(256, arr.nbytes + 256))
        owned.append(d)
        d.zero()
        if arr.nbytes:
            d.upload(arr)
        return d

    started = False
    try:
        state, arena = guarded(lay["total"]), guarded(arena_bytes)
        side = {t: guarded(sizes[t] * cap) for t in SIDES}
        for t in SIDES:
            abi._check(abi.lib().bt_memset_d(ctx.h, side[t].ptr, 0, sizes[t] * cap))
        abi._check(abi.lib().bt_memset_d(ctx.h, arena.ptr, 0xA5, arena_bytes))

        def snapshot(live):
            """Where a checkpoint's state and side tables are read from: the live buffers, or copies made in stream order."""
            if live:
                return state, side
            c_state, c_side = guarded(lay["total"]), {t: guarded(sizes[t] * cap) for t in SIDES}
            calls.append(lambda: copy_d2d(c_state.ptr, state.ptr, lay["total"], stream))
            for t in SIDES:
                calls.append(lambda t=t: copy_d2d(c_side[t].ptr, side[t].ptr, sizes[t] * cap, stream))
            return c_state, c_side

        for j, o in enumerate(scn.ops):
            if o["op"] == "batch":
                n = len(o["frames"])
                nw = (n + 63) // 64
                data, desc = sc.pack(o["frames"])
                if fmt == "xdp":   # struct xdp_desc {u64 addr; u32 len; u32 options}
                    x = np.zeros((max(n, 1), 2), np.uint64)
                    x[:n, 0], x[:n, 1] = desc & fr.MASK48, desc >> np.uint64(48) | np.uint64(0xABCD0000 << 32)
                    desc = x.reshape(-1)
                d_data, d_desc = upload(data), upload(desc)
                batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, len(data), abi.DESC_XDP if fmt == "xdp" else abi.DESC_PACKED, 0)
                d_sel = None if o["select"] is None or not n else upload(sc.words(o["select"], rng))
                d_hit = upload(sc.words(o["hit"], rng)) if n else None
                d_ts = upload(o["ts"]) if n else None
                b = {"flow_id": guarded(4 * n), "seq": guarded(4 * n), "byte_off": guarded(8 * n), "seq_words": guarded(8 * nw),
                     "msel_words": guarded(8 * nw), "res": guarded(64 * len(RESULTS))}
                res = {name_: b["res"].ptr + 64 * i for i, (name_, _) in enumerate(RESULTS)}

                def chain(o=o, n=n, batch=batch, b=b, res=res, d_sel=d_sel, d_hit=d_hit, d_ts=d_ts):
                    fid = b["flow_id"].ptr
                    ctx.flow_track_update(state.ptr, batch, arena.ptr, abi.flow_track_scratch_bytes(n), res["track"], select=d_sel, ts=d_ts,
                                          flow_id=fid, stream=stream)
                    ctx.flow_tcp_update(batch, fid, flags, side["tcp"].ptr, cap, res["tcp"], stream=stream)
                    ctx.flow_stat_update(batch, fid, flags, side["stat"].ptr, cap, res["stat"], ts=d_ts, stream=stream)
                    ctx.flow_mark_update(batch, fid, d_hit, o["mark"], side["mark"].ptr, cap, res["mark"], ts=d_ts, stream=stream)
                    ctx.flow_seq(batch, fid, d_sel, side["seq"].ptr, cap, arena.ptr, abi.flow_seq_scratch_bytes(n, cap), res["seq_res"],
                                 max_packets=o["mp"], max_bytes=o["mb"], flags=o["seq_flags"], seq=b["seq"].ptr, byte_off=b["byte_off"].ptr,
                                 out_select=b["seq_words"].ptr, stream=stream)
                    ctx.flow_mark_select(fid, n, side["mark"].ptr, cap, o["sel_mask"], b["msel_words"].ptr, res["msel"], op=o["sel_op"],
                                         flags=o["sel_flags"], base=b["seq_words"].ptr, stream=stream)
                calls.append(chain)

                def read_batch(b=b):
                    raw = b["res"].read()
                    got = {name_: cls.from_bytes(raw[64 * i:]).as_dict() for i, (name_, cls) in enumerate(RESULTS)}
                    got.update({"flow_id": b["flow_id"].read(np.uint32), "seq": b["seq"].read(np.uint32), "byte_off": b["byte_off"].read(np.uint64),
                                "seq_words": b["seq_words"].read(np.uint64), "msel_words": b["msel_words"].read(np.uint64)})
                    return got
                readers.append(read_batch)
            elif o["op"] == "expire":
                c = o["cap"]
                e = {"remap": guarded(4 * cap), "res": guarded(32), "track": guarded(104 * c) if c is not None else None}
                for t in SIDES:
                    e[t] = guarded(sizes[t] * c) if c is not None else None
                at = lambda g: g.ptr if g is not None else None  # noqa: E731

                def expire(o=o, e=e, c=c, at=at):
                    if o["closed_idle"] is None:
                        ctx.flow_track_expire(state.ptr, o["now"], o["idle"], arena.ptr, abi.flow_track_expire_scratch_bytes(cap), e["res"].ptr,
                                              expired=at(e["track"]), expired_cap=c or 0, remap=e["remap"].ptr, stream=stream)
                        moved = SIDES
                    else:   # the TCP table goes with the expire itself
                        ctx.flow_track_expire_tcp(state.ptr, o["now"], o["idle"], o["closed_idle"], side["tcp"].ptr, arena.ptr,
                                                  abi.flow_track_expire_tcp_scratch_bytes(cap), e["res"].ptr, expired=at(e["track"]),
                                                  expired_cap=c or 0, expired_tcp=at(e["tcp"]), remap=e["remap"].ptr, stream=stream)
                        moved = SIDES[1:]
                    for t in moved:   # each with its own expired_side
                        ctx.flow_track_side_move(side[t].ptr, sizes[t], cap, e["remap"].ptr, e["res"].ptr, arena.ptr,
                                                 abi.flow_track_side_move_scratch_bytes(cap, sizes[t]), expired_side=at(e[t]),
                                                 expired_cap=c or 0, stream=stream)
                calls.append(expire)

                def read_expire(e=e, c=c, j=j):
                    res = abi.FlowTrackExpireResult.from_bytes(e["res"].read()).as_dict()
                    remap = e["remap"].read(np.uint32)
                    nb, ne = res["n_flows_before"], res["n_expired"]
                    assert (remap[nb:] == np.uint32(0x01010101 * POISON)).all(), f"op {j}: remap written at or past n_flows_before"
                    got = {"result": res, "remap": remap[:nb]}
                    for t, dt in (("track", sm.FLOW_TRACK_REC),) + tuple(SIDE_DTYPES.items()):
                        if c is None:
                            got[t] = None
                            continue
                        raw = e[t].read()
                        assert ne <= c and (raw[dt.itemsize * ne:] == POISON).all(), f"op {j}: expired {t} written at or past n_expired"
                        got[t] = raw[:dt.itemsize * ne].view(dt)
                    return got
                readers.append(read_expire)
            else:
                last = j == len(scn.ops) - 1
                if stream is None and not last:
                    readers.append(lambda: None)
                    continue
                s_state, s_side = snapshot(last)
                v = {"hosts": guarded(128 * scn.host_cap), "ends": guarded(8 * cap), "hres": guarded(64)}
                for m in range(5):
                    v[m] = {"ids": guarded(4 * k), "values": guarded(8 * k), "recs": guarded(104 * k), "tcps": guarded(16 * k), "res": guarded(48)}

                def views(v=v):
                    for m in range(5):
                        ctx.flow_track_top(state.ptr, m, k, arena.ptr, abi.flow_track_top_scratch_bytes(cap, k), v[m]["res"].ptr,
                                           top_id=v[m]["ids"].ptr, top_value=v[m]["values"].ptr, top=v[m]["recs"].ptr, tcp=side["tcp"].ptr,
                                           top_tcp=v[m]["tcps"].ptr, stream=stream)
                    ctx.flow_track_hosts(state.ptr, scn.host_cap, arena.ptr, abi.flow_track_hosts_scratch_bytes(cap, 0), v["hres"].ptr,
                                         hosts=v["hosts"].ptr, endpoint_host=v["ends"].ptr, tcp=side["tcp"].ptr, stream=stream)
                calls.append(views)

                def read_check(v=v, s_state=s_state, s_side=s_side, j=j):
                    raw = s_state.read()
                    assert (raw[128:lay["records"]] == POISON).all() and (raw[lay["records"] + 104 * cap:lay["slot_words"]] == POISON).all()
                    got = {"hdr": abi.FlowTrackHdr.from_bytes(raw).as_dict(),
                           "track": raw[lay["records"]:lay["records"] + 104 * cap].copy().view(sm.FLOW_TRACK_REC), "top": {}}
                    for t in SIDES:
                        got[t] = s_side[t].read().view(SIDE_DTYPES[t])
                    for m in range(5):
                        res = abi.FlowTopResult.from_bytes(v[m]["res"].read()).as_dict()
                        nt = res["n_top"]
                        got["top"][m] = {"result": res}
                        for f, dt in (("ids", np.dtype(np.uint32)), ("values", np.dtype(np.uint64)), ("recs", sm.FLOW_TRACK_REC),
                                      ("tcps", abi.FlowTcpRec)):
                            raw_v = v[m][f].read()
                            assert nt <= k and (raw_v[dt.itemsize * nt:] == POISON).all(), f"op {j}: top {f} written at or past n_top"
                            got["top"][m][f] = raw_v[:dt.itemsize * nt].view(dt)
                    res = abi.FlowHostsResult.from_bytes(v["hres"].read()).as_dict()
                    hosts, ends = v["hosts"].read(), v["ends"].read()
                    nh, nf = res["n_written"], res["n_flows"]
                    assert (hosts[128 * nh:] == POISON).all() and (ends[8 * nf:] == POISON).all(), f"op {j}: hosts written past their counts"
                    got["hosts"] = {"hosts": hosts[:128 * nh].view(abi.FlowHostRec), "endpoint_host": ends[:8 * nf].view(np.uint32), "result": res}
                    return got
                readers.append(read_check)

        ctx.synchronize()   # the uploads and the poison are in place
        ctx.flow_track_init(state.ptr, lay["total"], cap, flags, scn.slots, stream=stream)
        started = True
        for call in calls:   # nothing but the calls themselves from here to the wait
            call()
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        arena.read()   # its guards
        return [r() for r in readers]
    finally:
        if started:
            abi.Context.flow_track_forget(state.ptr)   # before the memory goes back
        for b in owned:
            b.free()


def both_streams(ctx, name, fmt="packed"):
    """On a stream of its own against the model, then on a second state and the context's stream: the same bytes."""
    st = ctx.stream_create()
    try:
        first = run_device(ctx, name, st, fmt)
    finally:
        ctx.stream_destroy(st)
    sc.compare(name, first, f"device ({fmt}): ")
    second = run_device(ctx, name, None, fmt)
    for j, (a, b) in enumerate(zip(first, second)):
        assert b is None or sc.same(a, b), f"{name} op {j}: two runs on two states and two streams differ"
    return first


@pytest.mark.parametrize("name", sc.SCENARIOS)
def test_the_device_chain_is_what_each_key_s_packets_add_up_to(gpu_ctx, name):
    sc.assert_not_vacuous(name)   # on the model alone, before anything is compared
    dev = both_streams(gpu_ctx, name)
    host = run_host(name)   # bit for bit: the header, the records, every side table and every output
    for j, (a, b) in enumerate(zip(dev, host)):
        assert sc.same(a, b), f"{name} op {j} ({sc.scenario(name).ops[j]['op']}): the device and the host form differ"


def test_xdp_descriptors(gpu_ctx):
    """churn's first four batches as XDP descriptors; the host form does not take them."""
    dev = both_streams(gpu_ctx, "xdp", "xdp")
    assert dev[-1]["hdr"]["n_flows"] > 0 and dev[-1]["hdr"]["seq"] == 4
