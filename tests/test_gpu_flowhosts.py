"""GPU: the endpoint table of a device-resident flow tracker (bt_flow_track_hosts_device,
beatrice_amd/csrc/bt_flowhosts.hip). Expected values come from the restatement in flowhosts_ref.py
(a dict group-by over the records), never from the code under test; the host form must agree bit
for bit. hosts, endpoint_host, the result and the scratch sit in poisoned buffers between two
256-byte guards, the outputs sized to exactly host_cap records and 2 flow_cap numbers, and are
compared whole, the poison behind n_written and 2 n_flows included; every call runs twice with
byte-equal outputs; the state and the side table are read back unchanged."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowhosts_ref as fh  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import flowtcp_ref as tr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import POISON, Guarded, Source, golden_keys  # noqa: E402
from test_gpu_flowtcp import packet_tcp  # noqa: E402
from test_gpu_flowtop import DevState  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = ftr.BIDIRECTIONAL
POISON32 = 0xC7C7C7C7


class Outs:
    """The outputs of one call (host_cap records, 2 flow_cap numbers), the result and the scratch, guarded and poisoned."""

    def __init__(self, ctx, cap, host_cap, slots=0):
        self.ctx, self.cap, self.host_cap, self.slots = ctx, cap, host_cap, slots
        self.need = abi.flow_track_hosts_scratch_bytes(cap, slots)
        self.hosts, self.ends = Guarded(ctx, 128 * host_cap), Guarded(ctx, 8 * cap)
        self.res, self.scratch = Guarded(ctx, 64), Guarded(ctx, self.need)
        self.all = (self.hosts, self.ends, self.res, self.scratch)

    def poison(self):
        for g in self.all:
            abi._check(abi.lib().bt_memset_d(self.ctx.h, g.buf.ptr, POISON, g.buf.nbytes))

    def read(self):
        """(result dict, hosts' bytes, endpoint_host's bytes); every guard, the scratch's too, is checked."""
        self.scratch.read()
        return abi.FlowHostsResult.from_bytes(self.res.read()).as_dict(), self.hosts.read().tobytes(), self.ends.read().tobytes()

    def free(self):
        for g in self.all:
            g.free()


def check_outputs(got, want, with_ends, where):
    res, hosts, ends = got
    if want["overflow"]:
        assert res["overflow_endpoints"] != 0 and (res["status"], res["n_flows"], res["slots"]) == (0, want["n_flows"], want["slots"]), \
            f"{where}: {res}"
        return
    assert res == want["result"], f"{where}: result {res} != {want['result']}"
    nw, nf = res["n_written"], res["n_flows"]
    assert hosts[:128 * nw] == want["hosts"].tobytes(), f"{where}: hosts"
    assert hosts[128 * nw:] == bytes([POISON]) * (len(hosts) - 128 * nw), f"{where}: hosts written behind n_written"
    if with_ends:
        assert ends[:8 * nf] == want["endpoint_host"].astype("<u4").tobytes(), f"{where}: endpoint_host"
        assert ends[8 * nf:] == bytes([POISON]) * (len(ends) - 8 * nf), f"{where}: endpoint_host written behind 2 n_flows"
    else:
        assert ends == bytes([POISON]) * len(ends), f"{where}: endpoint_host written without being asked for"


def call_twice(ctx, state, tcp, o, with_ends, want, where, stream=None):
    """One query into poisoned outputs, twice: both runs equal `want` whole and each other."""
    runs = []
    for _ in range(2):
        o.poison()
        ctx.synchronize()
        ctx.flow_track_hosts(state, o.host_cap, o.scratch.ptr, o.need, o.res.ptr, hosts=o.hosts.ptr if o.host_cap else None,
                             endpoint_host=o.ends.ptr if with_ends else None, tcp=tcp, slots=o.slots, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        runs.append(o.read())
        check_outputs(runs[-1], want, with_ends, where)
    if not want["overflow"]:
        assert runs[0] == runs[1], f"{where}: two runs differ"
    return runs[0]


def host_state(cap, flags, n_flows, recs):
    t = abi.HostFlowTracker(cap, flags)
    t.state[:128] = np.frombuffer(fh.header(flags, cap, t.layout["slots"], n_flows), np.uint8)
    t.state[t.layout["records"]:t.layout["records"] + 104 * cap] = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    return t


def host_agrees(host, tcp, o, with_ends, got, where):
    """The host form under the same options: result, records and numbers bit for bit."""
    hosts, ends, res = abi.flow_track_hosts_host(host.state, o.host_cap, o.slots, tcp)
    assert res == got[0], f"{where}: the host form's result {res}"
    assert hosts.tobytes() == got[1][:128 * res["n_written"]], f"{where}: the host form's records"
    assert not with_ends or ends.astype("<u4").tobytes() == got[2][:8 * res["n_flows"]], f"{where}: the host form's host numbers"


def run_table(ctx, name, cap, pairs, flags=FLAGS, variants=None):
    """One crafted table on the device under every variant (host_cap, slots, with tcp, with endpoint_host)."""
    n = len(pairs)
    recs, tcp = fh.craft(cap, pairs)
    dev = DevState(ctx, cap, flags)
    host = host_state(cap, flags, n, recs)
    n_hosts = fh.expected(recs[:n], None, flags, 0, 1 << 31)["result"]["n_hosts"]
    variants = variants or [(2 * cap, 0, True, True), (n_hosts + 3, 0, False, True), (max(0, n_hosts - 1) // 2, 0, True, False),
                            (0, 0, True, True)]
    try:
        before = dev.load(n, recs, tcp, hdr=fh.header(flags, cap, dev.lay["slots"], n))
        for host_cap, slots, with_tcp, with_ends in variants:
            o = Outs(ctx, cap, host_cap, slots)
            try:
                where = f"{name} cap={cap} n={n} host_cap={host_cap} slots={slots} tcp={with_tcp} ends={with_ends}"
                want = fh.expected(recs[:n], tcp if with_tcp else None, flags, host_cap, slots or fh.auto_slots(cap))
                got = call_twice(ctx, dev.state.ptr, dev.tcp.ptr if with_tcp else None, o, with_ends, want, where)
                if not want["overflow"]:
                    host_agrees(host, tcp if with_tcp else None, o, with_ends, got, where)
            finally:
                o.free()
        assert dev.unchanged(before), f"{name}: the state or the side table was written"
    finally:
        dev.free()
    return n_hosts


@pytest.mark.parametrize("case", fh.crafted(), ids=lambda c: c[0])
def test_crafted_tables(gpu_ctx, case):
    run_table(gpu_ctx, *case)


def test_without_the_side_table_the_tcp_fields_are_zero(gpu_ctx):
    """tcp == NULL: nothing of a side table is read (there is none to read) and the TCP fields stay 0."""
    ctx, cap = gpu_ctx, 300
    pairs = fh.pairs_pool(257, 50, 9)
    recs, _ = fh.craft(cap, pairs)
    dev, o = DevState(ctx, cap, 0), Outs(ctx, cap, 2 * cap)
    try:
        dev.load(257, recs, np.zeros(cap, tr.TCP_REC), hdr=fh.header(0, cap, dev.lay["slots"], 257))
        got = call_twice(ctx, dev.state.ptr, None, o, True, fh.expected(recs[:257], None, 0, 2 * cap, fh.auto_slots(cap)), "no tcp")
        hosts = np.frombuffer(got[1][:128 * got[0]["n_written"]], fh.HOST_REC)
        assert got[0]["n_written"] > 50 and not hosts["tcp_state"].any() and not hosts["syn_flows"].any() and not hosts["syn_packets"].any()
    finally:
        o.free()
        dev.free()


def test_slots_exactly_the_hosts_and_below(gpu_ctx):
    """Load 1.0 succeeds; one slot's worth of hosts too many overflows, with nothing out of bounds."""
    ctx = gpu_ctx
    run_table(ctx, "128 hosts in 128 slots", 64, fh.pairs_fresh(64), variants=[(128, 128, True, True)])
    run_table(ctx, "512 hosts in 512 slots", 256, fh.pairs_fresh(256), variants=[(512, 512, True, True), (100, 512, False, False)])
    run_table(ctx, "514 hosts in 512 slots", 257, fh.pairs_fresh(257), variants=[(514, 512, True, True)])
    run_table(ctx, "514 hosts in 128 slots", 300, fh.pairs_fresh(257), variants=[(600, 128, True, True), (7, 128, False, False)])


def test_unidirectional_tracker_flags(gpu_ctx):
    """Without BT_FLOWTAB_BIDIRECTIONAL the connection state is decided from flags[0] alone."""
    run_table(gpu_ctx, "unidirectional", 130, fh.pairs_pool(130, 20, 3), flags=0)
    run_table(gpu_ctx, "l3 only", 130, fh.pairs_pool(130, 20, 4), flags=ftr.L3_ONLY | FLAGS)


def hub_and_pool(ctx, cap, where):
    """A table of `cap` flows, all live: a hub in every flow in alternating roles, the other endpoints
    repeating every 1,000 flows and 300 fresh hosts at the end, so that the restatement stays small
    (1,301 hosts) while every block of every kernel has work. The side table and endpoint_host are
    given and host_cap is above n_hosts; the outputs are compared whole with the restatement, twice,
    and with the host form."""
    n = cap
    recs, tcp = np.zeros(cap, fkr.FLOW_TRACK_REC), np.zeros(cap, tr.TCP_REC)
    f = np.arange(n, dtype=np.uint32)
    other = (np.uint32(0x0B000000) + f % np.uint32(1000)).astype(">u4").view(np.uint8).reshape(-1, 4)
    late = f >= cap - 300                                  # the last block and a bit: 300 fresh hosts
    other[late] = (np.uint32(0x0C000000) + f[late]).astype(">u4").view(np.uint8).reshape(-1, 4)
    hub = np.frombuffer(fh.v4(0xC0A80001), np.uint8)
    even = (f % 2 == 0)[:, None]
    recs["key"][:, 0:4], recs["key"][:, 4:8] = np.where(even, hub, other), np.where(even, other, hub)
    recs["klass"] = fh.V4
    recs["packets"][:, 0], recs["packets"][:, 1] = f % 7, 1
    recs["bytes"][:, 0], recs["bytes"][:, 1] = f.astype(np.uint64) * np.uint64(3), 64
    recs["first_ts"], recs["last_ts"] = 10 + f % 13, 50 + f % 17
    tcp["flags"][:, 0], tcp["flags"][:, 1] = 0x12, np.where(f % 3 == 0, 0x10, 0x02)
    tcp["syn_packets"] = 1
    dev, o = DevState(ctx, cap, FLAGS), Outs(ctx, cap, 2000)
    try:
        before = dev.load(n, recs, tcp, hdr=fh.header(FLAGS, cap, dev.lay["slots"], n))
        want = fh.expected(recs, tcp, FLAGS, 2000, fh.auto_slots(cap))
        assert want["result"]["n_hosts"] == 1301 and want["hosts"]["first_flow"][-1] == cap - 1
        got = call_twice(ctx, dev.state.ptr, dev.tcp.ptr, o, True, want, where)
        host_agrees(host_state(cap, FLAGS, n, recs), tcp, o, True, got, where)
        assert dev.unchanged(before)
    finally:
        o.free()
        dev.free()


def test_one_past_the_scan_span(gpu_ctx):
    """flow_cap one past 1,024 blocks of 256 flows: the one-block scan gives a thread two blocks."""
    hub_and_pool(gpu_ctx, 1024 * 256 + 1, "one past the scan span")


def test_one_past_the_sum_grid(gpu_ctx):
    """flow_cap one past 2,048 blocks of 256 flows: bt_flowhosts_sum's grid-stride loop runs a second
    time in block 0 (the block's LDS cache and tags carry over, the partial is the tile's, not the
    block's), and the hub's and the pool's sums come from more than one tile per block."""
    hub_and_pool(gpu_ctx, 2048 * 256 + 1, "one past the sum grid")


def test_a_header_that_is_not_this_tracker_gives_status_1_and_nothing_else(gpu_ctx):
    ctx, cap, n = gpu_ctx, 300, 257
    pairs = fh.pairs_pool(n, 50, 2)
    recs, tcp = fh.craft(cap, pairs)
    dev, o = DevState(ctx, cap, FLAGS), Outs(ctx, cap, 100)
    zero = {"n_flows": 0, "n_hosts": 0, "n_written": 0, "status": 1, "overflow_endpoints": 0, "slots": 0, "hosts_v4": 0, "hosts_v6": 0,
            "packets_total": 0, "bytes_total": 0, "reserved": [0, 0]}
    try:
        slots = dev.lay["slots"]
        for what, hdr in (("magic", b"XXXX" + fh.header(FLAGS, cap, slots, n)[4:]), ("flags", fh.header(0, cap, slots, n)),
                          ("flow_cap", fh.header(FLAGS, cap + 1, slots, n)), ("slots", fh.header(FLAGS, cap, 2 * slots, n)),
                          ("n_flows above flow_cap", fh.header(FLAGS, cap, slots, cap + 1))):
            before = dev.load(n, recs, tcp, hdr=hdr)
            want = {"overflow": False, "result": zero, "hosts": np.zeros(0, fh.HOST_REC), "endpoint_host": np.zeros(0, np.uint32)}
            call_twice(ctx, dev.state.ptr, dev.tcp.ptr, o, True, want, what)
            assert dev.unchanged(before)
        before = dev.load(n, recs, tcp, hdr=fh.header(FLAGS, cap, slots, n))   # the right header again
        call_twice(ctx, dev.state.ptr, dev.tcp.ptr, o, True, fh.expected(recs[:n], tcp, FLAGS, 100, fh.auto_slots(cap)), "right header")
        assert dev.unchanged(before)
    finally:
        o.free()
        dev.free()


def test_refusals_that_need_a_known_state(gpu_ctx):
    ctx, cap = gpu_ctx, 64
    dev, o = DevState(ctx, cap, FLAGS), Outs(ctx, cap, 8)
    try:
        for nbytes, slots in ((o.need - 1, 0), (abi.flow_track_hosts_scratch_bytes(cap, 128), 1024), (0, 0)):
            with pytest.raises(abi.BtError, match="scratch_bytes"):
                ctx.flow_track_hosts(dev.state.ptr, 8, o.scratch.ptr, nbytes, o.res.ptr, hosts=o.hosts.ptr, slots=slots)
        with pytest.raises(abi.BtError, match="null hosts"):
            ctx.flow_track_hosts(dev.state.ptr, 8, o.scratch.ptr, o.need, o.res.ptr)
        abi.Context.flow_track_forget(dev.state.ptr)
        with pytest.raises(abi.BtError, match="not an initialised tracker"):
            ctx.flow_track_hosts(dev.state.ptr, 8, o.scratch.ptr, o.need, o.res.ptr, hosts=o.hosts.ptr)
        ctx.flow_track_init(dev.state.ptr, dev.lay["total"], cap, FLAGS)
        ctx.synchronize()
        assert o.read()[0]["n_flows"] == POISON32   # no refused call wrote anything
    finally:
        o.free()
        dev.free()


def test_random_sweep_of_small_tables(gpu_ctx):
    """A few hundred seeded tables: host pools of 1, 3, 50 and n; sizes around the wave and the block;
    host_cap, slots, the side table and endpoint_host rotate."""
    ctx = gpu_ctx
    rng = np.random.default_rng(20261020)
    for cap in (70, 300):
        dev = DevState(ctx, cap, FLAGS)
        outs = {}
        try:
            for t in range(120):
                n = int(rng.integers(0, cap + 1))
                pool = (1, 3, 50, max(1, n))[t % 4]
                pairs = fh.pairs_pool(n, pool, 1000 * cap + t)
                recs, tcp = fh.craft(cap, pairs, seed=t)
                before = dev.load(n, recs, tcp, hdr=fh.header(FLAGS, cap, dev.lay["slots"], n))
                host_cap, slots = (2 * cap, 0, 5, 40)[(t // 4) % 4], (0, 1024)[(t // 16) % 2]
                with_tcp, with_ends = t % 3 != 0, t % 5 != 0
                if (host_cap, slots) not in outs:
                    outs[(host_cap, slots)] = Outs(ctx, cap, host_cap, slots)
                o = outs[(host_cap, slots)]
                where = f"sweep cap={cap} t={t} n={n} pool={pool} host_cap={host_cap} slots={slots}"
                want = fh.expected(recs[:n], tcp if with_tcp else None, FLAGS, host_cap, slots or fh.auto_slots(cap))
                got = call_twice(ctx, dev.state.ptr, dev.tcp.ptr if with_tcp else None, o, with_ends, want, where)
                host_agrees(host_state(cap, FLAGS, n, recs), tcp if with_tcp else None, o, with_ends, got, where)
                assert dev.unchanged(before), where
        finally:
            for o in outs.values():
                o.free()
            dev.free()


@pytest.mark.parametrize("name,cap,flags", [("c3", 5000, FLAGS), ("fuzz", 700, 0)])
def test_end_to_end_behind_the_updates_on_one_stream(gpu_ctx, name, cap, flags):
    """A golden and half of it again through bt_flow_track_update_device in 3 batches with the side table
    behind each, an expire of the first batch's idle flows in the middle, all on one non-default stream,
    and the query enqueued behind them with no wait in between; against the restatement over
    flowtrack_ref / flowtcp_ref."""
    ctx = gpu_ctx
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    n = n0 + n0 // 2
    desc, reps = np.resize(g["desc"], n), np.resize(np.arange(n0), n)
    keys = golden_keys(name, False)
    tcp, fl, dirs = packet_tcp(name, False, flags)
    ref, want_tcp = fkr.Tracker(cap, flags), np.zeros(cap, tr.TCP_REC)
    dev = DevState(ctx, cap, flags)
    abi._check(abi.lib().bt_memset_d(ctx.h, dev.tcp.ptr, 0, 16 * cap))
    ctx.synchronize()
    o = Outs(ctx, cap, 2 * cap)
    st = ctx.stream_create()
    bufs, srcs = [], []
    try:
        bounds = np.linspace(0, n, 4).astype(int)
        for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            r = reps[lo:hi]
            src = Source(ctx, name, hi - lo, "packed", desc=desc[lo:hi])
            need = abi.flow_track_scratch_bytes(hi - lo)
            ids, res, scratch, tres = Guarded(ctx, 4 * (hi - lo)), Guarded(ctx, 64), Guarded(ctx, need), Guarded(ctx, 32)
            srcs.append(src)
            bufs += [ids, res, scratch, tres]
            wid = ref.update(keys[0][r], keys[1][r], keys[2][r], src.lens, None, None, 10 * b)["flow_id"]
            tr.update(want_tcp, wid, tcp[r], fl[r], dirs[r])
            ctx.flow_track_update(dev.state.ptr, src.batch, scratch.ptr, need, res.ptr, batch_ts=10 * b, flow_id=ids.ptr, stream=st)
            ctx.flow_tcp_update(src.batch, ids.ptr, flags, dev.tcp.ptr, cap, tres.ptr, stream=st)
            if b == 1:   # the flows last seen in batch 0 leave, the side table moves with the others
                xneed = abi.flow_track_expire_tcp_scratch_bytes(cap)
                xs, xr = Guarded(ctx, xneed), Guarded(ctx, 32)
                bufs += [xs, xr]
                tr.expire(ref, want_tcp, 10, 5, (1 << 64) - 1)
                ctx.flow_track_expire_tcp(dev.state.ptr, 10, 5, (1 << 64) - 1, dev.tcp.ptr, xs.ptr, xneed, xr.ptr, stream=st)
        ctx.flow_track_hosts(dev.state.ptr, o.host_cap, o.scratch.ptr, o.need, o.res.ptr, hosts=o.hosts.ptr, endpoint_host=o.ends.ptr,
                             tcp=dev.tcp.ptr, stream=st)
        ctx.stream_synchronize(st)
        ctx.synchronize()
        recs = ref.records()
        assert len(recs) > 20
        want = fh.expected(recs, want_tcp, flags, o.host_cap, fh.auto_slots(cap))
        got = o.read()
        check_outputs(got, want, True, name)
        hosts = want["hosts"]
        assert int(hosts["packets"][:, 0].sum()) == want["result"]["packets_total"] == int(recs["packets"].sum())
        assert (hosts["tcp_state"].sum(axis=1) == hosts["flows"].sum(axis=1)).all() and (np.diff(hosts["first_flow"].astype(np.int64)) >= 0).all()
        assert dev.tcp.read().tobytes() == want_tcp.tobytes()
    finally:
        ctx.stream_destroy(st)
        for b in bufs + srcs + [o]:
            b.free()
        dev.free()
