"""The TCP side table's expected values, restated in numpy / Python and independent of the code
under test. Which packets contribute and their flags byte come from the goldens' reference-made
bt_rec (ok & L_TCP at byte 25, the IPv4 flags / fragment offset at bytes 38..39, tcp.flags at byte
81) or, for crafted and cut frames, from a Python walk of DESIGN.md §2; the direction comes from
flow_ref's key and flowtab_ref.canonical; the state function and the TCP-aware expire are restated
here. Every output of bt_flow_tcp_update_* and bt_flow_track_expire_tcp_* comes out of this file."""
import numpy as np

import flow_ref as fr
import flowtab_ref as ftr
import flowtrack_ref as fkr

FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
NONE, OPENING, ESTABLISHED, CLOSING, CLOSED, RESET, MIDSTREAM = range(7)
SENTINELS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB)

TCP_REC = np.dtype({
    "names": ["flags", "pad", "syn_packets", "fin_packets", "rst_packets"],
    "formats": [("u1", 2), ("u1", 2), "<u4", "<u4", "<u4"],
    "offsets": [0, 2, 4, 8, 12],
    "itemsize": 16,
})


def state(fwd: int, rev: int, table_flags: int = 0) -> int:
    """bt_flow_tcp_state: a function of the two unions, decided in this order."""
    u = fwd | rev
    bidir = bool(table_flags & ftr.BIDIRECTIONAL)
    if u == 0:
        return NONE
    if u & RST:
        return RESET
    if (fwd & rev & FIN) if bidir else (fwd & FIN):
        return CLOSED
    if u & FIN:
        return CLOSING
    if not u & SYN:
        return MIDSTREAM
    if (fwd & rev & SYN) if bidir else (fwd & SYN and fwd & ACK):
        return ESTABLISHED
    return OPENING


def tcp_of_rec(rec: np.ndarray):
    """(contributes [n] bool, flags byte [n]) of bt_rec rows: a parsed TCP layer and no IPv4 fragment."""
    rec = np.ascontiguousarray(rec).reshape(-1, 96)
    ok = rec[:, 25]
    frag = ((ok & fr.L_IPV4) != 0) & (((rec[:, 38].astype(np.int64) | (rec[:, 39].astype(np.int64) << 8)) & 0x3FFF) != 0)
    tcp = ((ok & fr.L_TCP) != 0) & ~frag
    return tcp, np.where(tcp, rec[:, 81], 0).astype(np.uint8)


def tcp_of_frame(frame: bytes):
    """DESIGN.md §2's walk over one frame as far as the TCP layer: (contributes, flags byte)."""
    n = len(frame)
    be16 = lambda o: (frame[o] << 8) | frame[o + 1]  # noqa: E731
    if n < 14:
        return False, 0
    et, k = be16(12), 0
    while k < 2 and et in (0x8100, 0x88A8):
        if n < 18 + 4 * k:
            return False, 0
        et = be16(16 + 4 * k)
        k += 1
    o3 = 14 + 4 * k
    if et == 0x0800:
        if n - o3 < 20 or frame[o3 + 9] != 6 or be16(o3 + 6) & 0x3FFF:
            return False, 0
        o4 = o3 + 4 * (frame[o3] & 0xF)
    elif et == 0x86DD:
        if n - o3 < 40 or frame[o3 + 6] != 6:
            return False, 0
        o4 = o3 + 40
    else:
        return False, 0
    if o4 > n or n - o4 < 20:
        return False, 0
    return True, frame[o4 + 13]


def tcp_of_frames(frames):
    got = [tcp_of_frame(bytes(f)) for f in frames]
    return np.array([g[0] for g in got], bool), np.array([g[1] for g in got], np.uint8)


def directions(inputs, nbytes, klass, table_flags: int) -> np.ndarray:
    """The flow table's direction of every packet: keys as flow_ref gives them under the table's L3_ONLY."""
    n = len(klass)
    out = np.zeros(n, np.int64)
    if table_flags & ftr.BIDIRECTIONAL:
        for i in range(n):
            out[i] = ftr.canonical(bytes(inputs[i, :nbytes[i]]), int(klass[i]))[1]
    return out


def update(table: np.ndarray, flow_id, tcp, flags, dirs) -> dict:
    """One batch added to `table` (TCP_REC, in place): the result dict of bt_flow_tcp_update_*."""
    flow_id = np.asarray(flow_id, np.uint32)
    cap = len(table)
    ok = flow_id < cap
    bad = int((~ok & ~np.isin(flow_id, np.array(SENTINELS, np.uint32))).sum())
    use = ok & np.asarray(tcp, bool)
    f, fl, d = flow_id[use].astype(np.int64), np.asarray(flags, np.uint8)[use], np.asarray(dirs, np.int64)[use]
    syn, fin, rst = ((fl & SYN) != 0) & ((fl & ACK) == 0), (fl & FIN) != 0, (fl & RST) != 0
    np.bitwise_or.at(table["flags"], (f, d), fl)
    for name, bit in (("syn_packets", syn), ("fin_packets", fin), ("rst_packets", rst)):
        add = np.zeros(cap, np.uint64)
        np.add.at(add, f[bit], 1)
        table[name] = (table[name].astype(np.uint64) + add).astype(np.uint32)   # mod 2^32
    return {"n": len(flow_id), "tcp_packets": int(use.sum()), "syn_packets": int(syn.sum()), "fin_packets": int(fin.sum()),
            "rst_packets": int(rst.sum()), "bad_ids": bad, "reserved": [0, 0]}


def expire(tracker: "fkr.Tracker", table: np.ndarray, now: int, idle: int, closed_idle: int, expired_cap=None) -> dict:
    """flowtrack_ref.Tracker.expire with one more way to leave; `table` (TCP_REC, flow_cap rows, in
    place) moves with the records. Adds "expired_tcp" to the plain expire's dict."""
    before = len(tracker.flows)

    def older(r, limit):
        return r["last_ts"] <= now and now - r["last_ts"] > limit

    leaving = []
    for f, r in enumerate(tracker.flows):
        s = state(int(table["flags"][f, 0]), int(table["flags"][f, 1]), tracker.flags)
        if older(r, idle) or (s in (CLOSED, RESET) and older(r, closed_idle)):
            leaving.append(f)
    gone = leaving if expired_cap is None else leaving[:expired_cap]
    gone_set = set(gone)
    remap = np.zeros(before, np.uint32)
    live, live_tcp = [], []
    for f, r in enumerate(tracker.flows):
        if f in gone_set:
            remap[f] = fkr.EXPIRED
        else:
            remap[f] = len(live)
            live.append(r)
            live_tcp.append(table[f].copy())
    expired = tracker._pack([tracker.flows[f] for f in gone])
    expired_tcp = table[gone].copy() if gone else np.zeros(0, TCP_REC)
    if gone:
        table[:before] = np.zeros(before, TCP_REC)
        if live_tcp:
            table[:len(live)] = np.array(live_tcp, TCP_REC)
    tracker.flows = live
    tracker.table = {(r["klass"], r["key"]): f for f, r in enumerate(live)}
    return {"expired": expired, "expired_tcp": expired_tcp, "remap": remap,
            "result": {"n_flows_before": before, "n_flows": len(live), "n_idle": len(leaving), "n_expired": len(gone),
                       "status": 0, "reserved": [0, 0, 0]}}
