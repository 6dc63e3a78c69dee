"""GPU: the device's layer walk (bt_flow_walk.h, under bt_fanout_keys, bt_flowtab_keys and
bt_flowtcp_update) held to the host's (flow_layers_host), which test_flow_walk.py holds to the
restatements. The truncation sweep of flow_walk_cases.py goes through bt_flow_fanout_device,
bt_flow_table_device and bt_flow_tcp_update_device; every output must be byte-equal to what the host
calls give. Then `bytes` ends at every offset of the last frame, a double-tagged IPv6 TCP frame
whose key, ports and flags byte lie at its very end: every byte at or past `bytes` reads as zero."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flow_walk_cases as wc  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import test_gpu_fanout as gfan  # noqa: E402
import test_gpu_flowtab as gtab  # noqa: E402
import test_gpu_flowtcp as gtcp  # noqa: E402
from beatrice_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def source(gpu_ctx):
    """The batch on the device, packed descriptors, zeros behind the data."""
    _, data, desc = wc.batch()
    src = gtab.Source(gpu_ctx, "c3", len(desc), data=data, desc=desc)
    yield src
    src.free()


def fanout_want(hashes, klass, lens):
    """Every output of the fan-out from the host's hashes and classes: the partition itself is flow_ref's."""
    return fr.expected(hashes, klass, lens, wc.QUEUES)


@pytest.mark.parametrize("l3_only", [False, True])
def test_device_fanout_equals_the_host(gpu_ctx, source, l3_only):
    h, klass, queue = wc.host_whole()["fanout"][l3_only]
    want = fanout_want(h, klass, source.lens)
    assert (want["queue"] == queue).all()   # all selected: the host's own queue bytes
    gfan.run(gpu_ctx, source.batch, source.n, wc.fanout_opts(l3_only), want, where=f"l3_only={l3_only}")


@pytest.mark.parametrize("flags", wc.ALL_FLAGS)
def test_device_table_and_tcp_update_equal_the_host(gpu_ctx, source, flags):
    n = source.n
    flow_id, flows, res = wc.host_whole()["table"][flags]
    gtab.run(gpu_ctx, source.batch, n, {"flow_id": flow_id, "flows": flows, "result": res}, flags, where=f"flags={flags}")
    table, tres = wc.host_whole()["tcp"][flags]
    d_ids = gtcp.upload(gpu_ctx, flow_id)
    try:
        gtcp.tcp_call(gpu_ctx, source.batch, n, d_ids.ptr, flags, n, table, tres, where=f"flags={flags}")
    finally:
        d_ids.free()


def test_bytes_at_every_offset_of_the_last_frame(gpu_ctx):
    """One set of buffers, one upload of the readable prefix per value of `bytes` (zeros behind it),
    the three calls on it, and the host forms with nbytes = bytes; the flags rotate with the cut."""
    frames, data, desc = wc.batch()
    n, start = len(frames), wc.last_frame_start()
    assert frames[-1] == wc.SEEDS["qinq_v6_tcp"] and start + 86 == len(data)
    lens = [len(f) for f in frames]
    L = abi.lib()
    sizes = {"data": len(data) + 256, "hash": 4 * n, "queue": n, "fres": 808, "ids": 4 * n, "flows": 80 * n, "tres": 72,
             "scratch": abi.flow_table_scratch_bytes(n, 0), "tcp": 16 * n, "tcpres": 32}
    d = {k: gpu_ctx.alloc(max(256, v)) for k, v in sizes.items()}
    d_desc = gtcp.upload(gpu_ctx, desc)

    def read(k, dtype=np.uint8):
        return d[k].download(np.zeros(sizes[k], np.uint8)).view(dtype)

    try:
        for cut in range(start, len(data) + 1):
            flags = wc.ALL_FLAGS[cut % 4]
            l3_only = bool(flags & ftr.L3_ONLY)
            where = f"bytes={cut} (the last frame's first {cut - start}) flags={flags}"
            d["data"].zero()
            d["data"].upload(data[:cut])
            abi._check(L.bt_memset_d(gpu_ctx.h, d["tcp"].ptr, 0, 16 * n))
            gpu_ctx.synchronize()
            batch = abi.Batch(d["data"].ptr, d_desc.ptr, 0, n, cut, abi.DESC_PACKED, 0)
            gpu_ctx.flow_fanout_device(batch, wc.fanout_opts(l3_only), d["fres"], hash=d["hash"], queue=d["queue"])
            gpu_ctx.flow_table_device(batch, abi.FlowTableOpts(flags, 0, n, 0), d["scratch"], sizes["scratch"], d["tres"],
                                      flow_id=d["ids"], flows=d["flows"])
            gpu_ctx.flow_tcp_update(batch, d["ids"], flags, d["tcp"], n, d["tcpres"])
            gpu_ctx.synchronize()
            # the host: the frames before the last are whole; the last has zeros from `bytes` on
            h, klass, queue = (a.copy() for a in wc.host_whole()["fanout"][l3_only])
            seen = frames[-1][:cut - start] + bytes(len(data) - cut)
            h[-1], klass[-1], queue[-1] = abi.flow_hash_host(seen, wc.fanout_opts(l3_only))
            assert (read("hash", np.uint32) == h).all() and (read("queue") == queue).all(), where
            assert abi.FanoutResult.from_bytes(read("fres")).as_dict() == fanout_want(h, klass, lens)["result"], where
            flow_id, flows, res = wc.host_table(flags, nbytes=cut)
            assert abi.FlowTableResult.from_bytes(read("tres")).as_dict() == res, where
            assert (read("ids", np.uint32) == flow_id).all(), where
            assert read("flows")[:80 * res["n_written"]].tobytes() == flows.tobytes(), where
            table, tcpres = wc.host_tcp(flags, flow_id, nbytes=cut)
            assert abi.FlowTcpResult.from_bytes(read("tcpres")).as_dict() == tcpres, where
            assert read("tcp").tobytes() == table.tobytes(), where
    finally:
        for b in list(d.values()) + [d_desc]:
            b.free()
