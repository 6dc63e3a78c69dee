"""The batch that holds the copies of the flow kernels' layer walk to each other (test_flow_walk.py,
test_gpu_flow_walk.py): seven seed frames, each emitted at every length from 0 to its own, packed
back to back so that frames start at every alignment; and every host call over it. The batch's last
frame is the double-tagged IPv6 TCP seed at full length."""
import functools

import numpy as np

import flowtab_ref as ftr
from beatrice_amd import abi

QUEUES = 8
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)

_MACS = bytes(range(1, 13))


def _tag(tpid, vid):
    return tpid.to_bytes(2, "big") + vid.to_bytes(2, "big")


def _v4(ihl, flags_frag, proto, total, host):
    """The 20 fixed bytes of an IPv4 header, 10.9.8.<host> -> 10.1.2.3: a flow of its own per seed."""
    return (bytes([0x40 | ihl, 0]) + total.to_bytes(2, "big") + b"\x12\x34" + flags_frag.to_bytes(2, "big") +
            bytes([64, proto, 0, 0, 10, 9, 8, host, 10, 1, 2, 3]))


def _v6(nh, plen, host, reverse=False):
    """An IPv6 header; source above destination as byte strings (direction 1), or with `reverse` below it."""
    hi, lo = bytes([0x20, 0x01, 0x0d, 0xb8] + list(range(40, 51)) + [host]), bytes([0x20, 0x01, 0x0d, 0xb8] + list(range(20, 32)))
    return b"\x60\x00\x00\x00" + plen.to_bytes(2, "big") + bytes([nh, 64]) + (lo + hi if reverse else hi + lo)


def _tcp(sp, dp, flags):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, flags]) + b"\xff\xff\x00\x00\x00\x00"


def _udp(sp, dp, ln):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + ln.to_bytes(2, "big") + b"\x00\x00"


def _pay(n):
    return bytes((37 * k + 11) & 0xFF for k in range(n))


SEEDS = {
    "v4_tcp_ihl6": _MACS + b"\x08\x00" + _v4(6, 0x4000, 6, 86, 1) + b"\x01\x01\x01\x00" + _tcp(443, 51000, 0x06) + _pay(42),
    "tag_v4_udp": _MACS + _tag(0x8100, 5) + b"\x08\x00" + _v4(5, 0, 17, 62, 2) + _udp(53, 3333, 42) + _pay(34),
    "v6_udp": _MACS + b"\x86\xdd" + _v6(17, 36, 3) + _udp(5353, 5353, 36) + _pay(28),
    "v4_fragment_mf": _MACS + b"\x08\x00" + _v4(5, 0x2000, 6, 66, 4) + _tcp(80, 40000, 0x10) + _pay(26),
    "v4_proto1": _MACS + b"\x08\x00" + _v4(5, 0, 1, 56, 5) + b"\x08\x00\x00\x00\x00\x01\x00\x02" + _pay(28),
    "three_tags": _MACS + _tag(0x88A8, 1) + _tag(0x8100, 2) + _tag(0x8100, 3) + b"\x08\x00" + _v4(5, 0, 17, 54, 6) + _udp(7, 9, 34) + _pay(26),
    "qinq_v6_tcp": _MACS + _tag(0x88A8, 100) + _tag(0x8100, 200) + b"\x86\xdd" + _v6(6, 24, 7, reverse=True) + _tcp(51000, 443, 0x19) + _pay(4),
}
assert list(SEEDS)[-1] == "qinq_v6_tcp"


@functools.lru_cache(maxsize=None)
def batch():
    """(frames, data, desc): every seed at every length 0 .. len(seed), in SEEDS' order, lengths ascending."""
    frames = [seed[:m] for seed in SEEDS.values() for m in range(len(seed) + 1)]
    offs = np.cumsum([0] + [len(f) for f in frames[:-1]])
    desc = np.array([int(o) | len(f) << 48 for o, f in zip(offs, frames)], np.uint64)
    data = np.frombuffer(b"".join(frames), np.uint8)
    assert 550 <= len(frames) <= 650 and frames[-1] == SEEDS["qinq_v6_tcp"] and int(offs[-1]) + len(frames[-1]) == len(data)
    return frames, data, desc


def last_frame_start():
    return int(batch()[2][-1] & np.uint64((1 << 48) - 1))


def fanout_opts(l3_only):
    return abi.FanoutOpts.make(QUEUES, abi.FANOUT_L3_ONLY if l3_only else 0)


def host_fanout(frames, l3_only):
    """bt_flow_hash_host over every frame: (hash [n] u32, class [n], queue [n] u8)."""
    opts = fanout_opts(l3_only)
    got = [abi.flow_hash_host(f, opts) for f in frames]
    return (np.array([g[0] for g in got], np.uint32), np.array([g[1] for g in got], np.int64),
            np.array([g[2] for g in got], np.uint8))


def host_table(flags, nbytes=None):
    """bt_flow_table_host over the batch with room for every flow: (flow_id, flows, result)."""
    frames, data, desc = batch()
    return abi.flow_table_host(data, desc, abi.FlowTableOpts(flags, 0, len(frames), 0), nbytes=nbytes)


def host_tcp(flags, flow_id, nbytes=None):
    """bt_flow_tcp_update_host into a zero side table of one record per packet: (table, result)."""
    frames, data, desc = batch()
    table = np.zeros(len(frames), abi.FlowTcpRec)
    return table, abi.flow_tcp_update_host(data, desc, flow_id, flags, table, nbytes=nbytes)


@functools.lru_cache(maxsize=None)
def host_whole():
    """Every host call over the whole batch, once: {"fanout": {l3_only: ...}, "table": {flags: ...}, "tcp": {flags: ...}}."""
    frames = batch()[0]
    table = {flags: host_table(flags) for flags in ALL_FLAGS}
    return {"fanout": {l3: host_fanout(frames, l3) for l3 in (False, True)}, "table": table,
            "tcp": {flags: host_tcp(flags, table[flags][0]) for flags in ALL_FLAGS}}
