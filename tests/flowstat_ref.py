"""The per-flow statistics side table's expected values, restated in numpy / Python and independent
of the code under test. What a frame contributes comes from a Python walk of DESIGN.md §2 over the
frame's bytes (at most two tags, no IPv6 extension headers, the flow key's fragment rule); the
direction comes from flow_ref's key and flowtab_ref.canonical as in flowtcp_ref; the reductions
are numpy's. Every output of bt_flow_stat_update_*, bt_flow_stat_rtt and
bt_flow_track_side_move_* comes out of this file."""
import numpy as np

import flowtcp_ref as tr
import flowtrack_ref as fkr

SEEN_TCP, SEEN_UDP, SEEN_ICMP, SEEN_ICMP6, SEEN_OTHER = 0x01, 0x02, 0x04, 0x08, 0x10
SEEN_FRAGMENT, SEEN_IP_OPTIONS, SEEN_VLAN, SEEN_L4 = 0x20, 0x40, 0x80, 0x100
U32, U64 = 0xFFFFFFFF, (1 << 64) - 1
SYN_STAMP, SYNACK_STAMP, ACK_STAMP, NO_STAMP = 0, 1, 2, 3
STAMP_FIELDS = ("syn_ts_c", "synack_ts_c", "ack_ts_c")

STAT_REC = np.dtype({
    "names": ["seen", "proto_max", "payload_packets", "ttl_max", "ttl_min_c", "len_max", "len_min_c", "payload_bytes", "len_sq",
              "syn_ts_c", "synack_ts_c", "ack_ts_c"],
    "formats": ["<u4", "<u4", ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u8", 2), ("<u8", 2), ("<u8", 2),
                ("<u8", 2), ("<u8", 2)],
    "offsets": [0, 4, 8, 16, 24, 32, 40, 48, 64, 80, 96, 112],
    "itemsize": 128,
})

FACTS = np.dtype([("ip", "?"), ("l4", "?"), ("tcp", "?"), ("seen", "<u4"), ("proto", "<u4"), ("ttl", "<u4"), ("len", "<u4"),
                  ("payload", "<u4"), ("stamp", "<u4")])


def facts_of_frame(frame: bytes):
    """What one frame contributes: a FACTS row as a tuple. `frame` holds the bytes the call may read
    (the caller has put zeros where `bytes` cut it); its length is the descriptor's."""
    n = len(frame)
    be16 = lambda o: (frame[o] << 8) | frame[o + 1]  # noqa: E731
    none = (False, False, False, 0, 0, 0, 0, 0, NO_STAMP)
    if n < 14:
        return none
    et, k = be16(12), 0
    while k < 2 and et in (0x8100, 0x88A8):
        if n < 18 + 4 * k:
            return none
        et = be16(16 + 4 * k)
        k += 1
    o3 = 14 + 4 * k
    seen = SEEN_VLAN if k else 0
    if et == 0x0800 and n - o3 >= 20:
        v4, proto, ttl, ihl = True, frame[o3 + 9], frame[o3 + 8], frame[o3] & 0xF
        o4 = o3 + 4 * ihl
        fragment = (be16(o3 + 6) & 0x3FFF) != 0
        ip_payload = be16(o3 + 2) - 4 * ihl
        seen |= (SEEN_FRAGMENT if fragment else 0) | (SEEN_IP_OPTIONS if ihl > 5 else 0)
    elif et == 0x86DD and n - o3 >= 40:
        v4, proto, ttl, o4, fragment = False, frame[o3 + 6], frame[o3 + 7], o3 + 40, False
        ip_payload = be16(o3 + 4)
    else:
        return none
    if proto == 6:
        seen |= SEEN_TCP
    elif proto == 17:
        seen |= SEEN_UDP
    elif v4 and proto == 1:
        seen |= SEEN_ICMP
    elif not v4 and proto == 58:
        seen |= SEEN_ICMP6
    else:
        seen |= SEEN_OTHER
    need = {6: 20, 17: 8}.get(proto, 0)
    l4 = bool(need) and not fragment and o4 <= n and n - o4 >= need
    tcp = l4 and proto == 6
    payload, stamp = 0, NO_STAMP
    if l4:
        seen |= SEEN_L4
        hdr = 4 * (frame[o4 + 12] >> 4) if tcp else 8
        payload = max(0, ip_payload - hdr)
    if tcp:
        fl = frame[o4 + 13]
        if fl & tr.SYN:
            stamp = SYNACK_STAMP if fl & tr.ACK else SYN_STAMP
        elif fl & tr.ACK and not fl & tr.RST:
            stamp = ACK_STAMP
    return (True, l4, tcp, seen, proto, ttl, min(n, 65535), payload, stamp)


def facts_of_frames(frames) -> np.ndarray:
    return np.array([facts_of_frame(bytes(f)) for f in frames], FACTS).reshape(-1)


def update(table: np.ndarray, flow_id, facts: np.ndarray, dirs, ts) -> dict:
    """One batch added to `table` (STAT_REC, in place): the result dict of bt_flow_stat_update_*.
    ts: one stamp per packet, or a scalar for the whole batch."""
    flow_id = np.asarray(flow_id, np.uint32)
    n, cap = len(flow_id), len(table)
    ts = np.broadcast_to(np.asarray(ts, np.uint64), (n,))
    ok = flow_id < cap
    bad = int((~ok & ~np.isin(flow_id, np.array(tr.SENTINELS, np.uint32))).sum())
    use = ok & facts["ip"]
    f, x, d, t = flow_id[use].astype(np.int64), facts[use], np.asarray(dirs, np.int64)[use], ts[use]
    np.bitwise_or.at(table["seen"], f, x["seen"] << (16 * d).astype(np.uint32))
    np.maximum.at(table["proto_max"], f, x["proto"])
    np.maximum.at(table["ttl_max"], (f, d), x["ttl"])
    np.maximum.at(table["ttl_min_c"], (f, d), ~x["ttl"])
    np.maximum.at(table["len_max"], (f, d), x["len"])
    np.maximum.at(table["len_min_c"], (f, d), ~x["len"])
    np.add.at(table["len_sq"], (f, d), x["len"].astype(np.uint64) ** 2)          # mod 2^64
    np.add.at(table["payload_bytes"], (f, d), x["payload"].astype(np.uint64))
    np.add.at(table["payload_packets"], (f, d), (x["payload"] > 0).astype(np.uint32))   # mod 2^32
    for kind, name in enumerate(STAMP_FIELDS):
        m = x["stamp"] == kind
        np.maximum.at(table[name], (f[m], d[m]), ~t[m])
    return {"n": n, "ip_packets": int(use.sum()), "l4_packets": int((use & facts["l4"]).sum()),
            "tcp_packets": int((use & facts["tcp"]).sum()), "bad_ids": bad, "reserved": [0, 0, 0]}


def rtt(rec) -> dict:
    """bt_flow_stat_rtt over one STAT_REC row."""
    syn_c, synack_c, ack_c = ([int(v) for v in rec[k]] for k in STAMP_FIELDS)
    out = {"has_initiator": 0, "initiator": 0, "server_valid": 0, "client_valid": 0, "rtt_server": 0, "rtt_client": 0}
    have = [c != 0 for c in syn_c]
    if not any(have):
        return out
    d = (1 if U64 - syn_c[1] < U64 - syn_c[0] else 0) if all(have) else have.index(True)
    out["has_initiator"], out["initiator"] = 1, d
    syn, synack, ack = U64 - syn_c[d], U64 - synack_c[1 - d], U64 - ack_c[d]
    if synack_c[1 - d] == 0 or synack < syn:
        return out
    out["server_valid"], out["rtt_server"] = 1, synack - syn
    if ack_c[d] == 0 or ack < synack:
        return out
    out["client_valid"], out["rtt_client"] = 1, ack - synack
    return out


def side_move(table: np.ndarray, remap, result: dict, expired_cap=None) -> np.ndarray:
    """bt_flow_track_side_move_*: `table` (any dtype, flow_cap rows, in place) through the expire that
    gave remap and result. Returns the expired flows' rows ([min(n_expired, expired_cap)])."""
    nb, nl = result["n_flows_before"], result["n_flows"]
    remap = np.asarray(remap, np.uint32)
    gone = [old for old in range(nb) if remap[old] == fkr.EXPIRED]
    out = table[gone[:len(gone) if expired_cap is None else expired_cap]].copy()
    if nl == nb:
        return out
    new = np.zeros(nb, table.dtype)
    for old in range(nb):
        if remap[old] != fkr.EXPIRED and remap[old] < nl:
            new[remap[old]] = table[old]
    table[:nb] = new
    return out
