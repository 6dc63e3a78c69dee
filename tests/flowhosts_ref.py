"""The endpoint table's expected values, restated in Python and independent of the code under test:
a dict group-by on (family, 16 address bytes) over the two endpoints of every record of a tracker,
in ascending contribution order c = 2 f + role, so that a dict's insertion order is the hosts'
numbering. Sums are Python ints reduced mod 2^64 / 2^32 at the end. Every output of
bt_flow_track_hosts_* comes out of expected(); crafted tables for both suites are built here too.
Nothing here calls the code under test."""
import struct

import numpy as np

import flowtcp_ref as tr
import flowtrack_ref as fkr

HOST_REC = np.dtype({
    "names": ["addr", "family", "pad", "first_flow", "flows", "packets", "bytes", "first_ts", "last_ts", "tcp_state", "syn_flows",
              "syn_packets", "fin_packets", "rst_packets"],
    "formats": [("u1", 16), "u1", ("u1", 3), "<u4", ("<u4", 2), ("<u8", 2), ("<u8", 2), "<u8", "<u8", ("<u4", 7), ("<u4", 2),
                "<u4", "<u4", "<u4"],
    "offsets": [0, 16, 17, 20, 24, 32, 48, 64, 72, 80, 108, 116, 120, 124],
    "itemsize": 128,
})
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
SYN = 0x02
NONE = 0xFFFFFFFF
V4, V4_L4, V6, V6_L4 = 1, 2, 3, 4


def auto_slots(flow_cap: int) -> int:
    s = 128
    while s < 4 * flow_cap:
        s <<= 1
    return s


def endpoint(rec, role: int):
    """(family, 16 address bytes) of a record's endpoint."""
    key = bytes(rec["key"])
    if int(rec["klass"]) in (V6, V6_L4):
        return 6, key[16 * role:16 * role + 16]
    return 4, key[4 * role:4 * role + 4] + bytes(12)


def expected(recs: np.ndarray, tcp, flags: int, host_cap: int, slots: int) -> dict:
    """recs: the n_flows live records; tcp: at least n_flows side records or None; flags: the
    tracker's. Returns hosts (HOST_REC rows, min(n_hosts, host_cap) of them), endpoint_host
    [2 n_flows] and the result dict. A table of fewer slots than hosts: "overflow" alone."""
    table = {}   # insertion order = order of first appearance
    ends = np.zeros(2 * len(recs), np.uint32)
    pk = by = 0
    # the columns as Python lists: plain ints, no numpy scalar in the loop
    keys, klass = [bytes(k) for k in recs["key"]], recs["klass"].tolist()
    packets, nbytes = recs["packets"].tolist(), recs["bytes"].tolist()
    first_ts, last_ts = recs["first_ts"].tolist(), recs["last_ts"].tolist()
    if tcp is not None:
        side = tcp[:len(recs)]
        tflags, tsyn, tfin, trst = side["flags"].tolist(), side["syn_packets"].tolist(), side["fin_packets"].tolist(), side["rst_packets"].tolist()
    for f in range(len(recs)):
        p, b = packets[f], nbytes[f]
        pk, by = pk + p[0] + p[1], by + b[0] + b[1]
        six = klass[f] in (V6, V6_L4)
        for role in (0, 1):
            who = (6, keys[f][16 * role:16 * role + 16]) if six else (4, keys[f][4 * role:4 * role + 4] + bytes(12))
            h = table.get(who)
            if h is None:
                h = table[who] = {"n": len(table), "first_flow": f, "flows": [0, 0], "packets": [0, 0], "bytes": [0, 0],
                                  "first_ts": first_ts[f], "last_ts": last_ts[f], "tcp_state": [0] * 7,
                                  "syn_flows": [0, 0], "syn": 0, "fin": 0, "rst": 0}
            ends[2 * f + role] = h["n"]
            h["flows"][role] += 1
            h["packets"][0] += p[role]; h["packets"][1] += p[1 - role]
            h["bytes"][0] += b[role]; h["bytes"][1] += b[1 - role]
            h["first_ts"], h["last_ts"] = min(h["first_ts"], first_ts[f]), max(h["last_ts"], last_ts[f])
            if tcp is not None:
                fl = tflags[f]
                h["tcp_state"][tr.state(fl[0], fl[1], flags)] += 1
                h["syn_flows"][0] += 1 if fl[role] & SYN else 0
                h["syn_flows"][1] += 1 if fl[1 - role] & SYN else 0
                h["syn"] += tsyn[f]; h["fin"] += tfin[f]; h["rst"] += trst[f]
    n_hosts = len(table)
    if n_hosts > slots:
        return {"overflow": True, "n_flows": len(recs), "slots": slots}
    nw = min(n_hosts, host_cap)
    hosts = np.zeros(nw, HOST_REC)
    for (family, addr), h in table.items():
        if h["n"] >= nw:
            continue
        o = hosts[h["n"]]
        o["addr"], o["family"], o["first_flow"] = np.frombuffer(addr, np.uint8), family, h["first_flow"]
        o["flows"] = h["flows"]
        o["packets"], o["bytes"] = [x & M64 for x in h["packets"]], [x & M64 for x in h["bytes"]]
        o["first_ts"], o["last_ts"] = h["first_ts"], h["last_ts"]
        o["tcp_state"], o["syn_flows"] = h["tcp_state"], h["syn_flows"]
        o["syn_packets"], o["fin_packets"], o["rst_packets"] = h["syn"] & M32, h["fin"] & M32, h["rst"] & M32
    res = {"n_flows": len(recs), "n_hosts": n_hosts, "n_written": nw, "status": 0, "overflow_endpoints": 0, "slots": slots,
           "hosts_v4": sum(1 for fam, _ in table if fam == 4), "hosts_v6": sum(1 for fam, _ in table if fam == 6),
           "packets_total": pk & M64, "bytes_total": by & M64, "reserved": [0, 0]}
    return {"overflow": False, "hosts": hosts, "endpoint_host": ends, "result": res}


# ---- crafted tables -------------------------------------------------------------------------

def header(flags: int, flow_cap: int, slots: int, n_flows: int, seq: int = 3) -> bytes:
    """A bt_flow_track_hdr (128 B)."""
    return struct.pack("<6I", fkr.MAGIC, flags, flow_cap, slots, n_flows, seq) + bytes(104)


def v4(x: int) -> bytes:
    return struct.pack(">I", x & 0xFFFFFFFF)


def v6(x: int) -> bytes:
    return (x & ((1 << 128) - 1)).to_bytes(16, "big")


def craft(flow_cap: int, pairs, seed: int = 0):
    """(records [flow_cap], side table [flow_cap]) whose first len(pairs) records have the endpoints
    pairs[f] = (a, b): two 4-byte strings (BT_FLOW_V4_L4, with ports) or two 16-byte ones
    (BT_FLOW_V6_L4). Counts, stamps and flags are seeded random, some sums close to 2^64 / 2^32; the
    records at or past len(pairs) hold garbage that must never be read as a flow."""
    rng = np.random.default_rng(seed * 7919 + 13 * flow_cap + len(pairs))
    n = len(pairs)
    recs, tcp = np.zeros(flow_cap, fkr.FLOW_TRACK_REC), np.zeros(flow_cap, tr.TCP_REC)
    for f, (a, b) in enumerate(pairs):
        six = len(a) == 16
        recs["key"][f, :2 * len(a)] = np.frombuffer(a + b, np.uint8)
        recs["key"][f, 2 * len(a):2 * len(a) + 4] = rng.integers(0, 256, 4)   # ports: never part of a host
        recs["klass"][f] = V6_L4 if six else V4_L4
    if n:
        recs["klass"][:n:5] -= 1   # every fifth flow without ports: BT_FLOW_V4 / BT_FLOW_V6
        big = rng.random(n) < 0.02
        recs["packets"][:n] = rng.integers(0, 1000, (n, 2))
        recs["bytes"][:n] = rng.integers(0, 1 << 20, (n, 2))
        recs["bytes"][:n, 0] = np.where(big, np.uint64(M64 - 5), recs["bytes"][:n, 0])
        recs["first_ts"][:n] = rng.integers(0, 1 << 40, n)
        recs["last_ts"][:n] = recs["first_ts"][:n] + rng.integers(0, 1 << 20, n).astype(np.uint64)
        recs["first"][:n], recs["last_batch"][:n] = rng.integers(0, 99, n), 2
        tcp["flags"][:n] = rng.choice([0, 0x02, 0x12, 0x10, 0x11, 0x14, 0x18, 0x1B], (n, 2))
        tcp["syn_packets"][:n] = np.where(big, M32 - 1, rng.integers(0, 4, n))
        tcp["fin_packets"][:n] = rng.integers(0, 3, n)
        tcp["rst_packets"][:n] = rng.integers(0, 2, n)
    for f in range(0, n, 5):   # the portless classes' port bytes are zero, as the tracker writes them
        a = 32 if recs["klass"][f] == V6 else 8
        recs["key"][f, a:a + 4] = 0
    recs["key"][n:] = 0xEE
    recs["klass"][n:] = V6_L4
    recs["packets"][n:], recs["bytes"][n:] = M64, M64 - 1
    recs["last_ts"][n:] = M64
    tcp["flags"][n:], tcp["syn_packets"][n:] = 0xFF, M32
    return recs, tcp


def pairs_fresh(n: int):
    """Every flow two fresh hosts."""
    return [(v4(0x0A000000 + 2 * f), v4(0x0A000001 + 2 * f)) for f in range(n)]


def pairs_hub(n: int, how: str):
    """One hub address in every flow: as role 0, as role 1, or alternating."""
    hub = v4(0xC0A80001)
    out = []
    for f in range(n):
        other = v4(0x0B000000 + f)
        first = how == "role0" or (how == "alternating" and f % 2 == 0)
        out.append((hub, other) if first else (other, hub))
    return out


def pairs_pool(n: int, pool: int, seed: int, mixed: bool = True):
    """Endpoints drawn from `pool` hosts, v4 and v6 mixed (a flow is of one family), some flows with
    both addresses equal; the pool holds 1.2.3.4 and 0102:0304:: whose first four bytes agree."""
    rng = np.random.default_rng(seed)
    p4 = [v4(0x01020304)] + [v4(0xAC100000 + int(x)) for x in rng.integers(0, 1 << 16, max(0, pool - 1))]
    p6 = [v6(0x01020304 << 96)] + [v6((0x20010DB8 << 96) + int(x)) for x in rng.integers(0, 1 << 16, max(0, pool - 1))]
    out = []
    for f in range(n):
        p = p6 if mixed and rng.random() < 0.3 else p4
        a = p[int(rng.integers(0, len(p)))]
        b = a if rng.random() < 0.05 else p[int(rng.integers(0, len(p)))]
        out.append((a, b))
    return out


def crafted():
    """[(name, flow_cap, pairs)]: the small tables both suites run. n_flows = len(pairs)."""
    out = [("empty", 64, [])]
    for cap in (1, 2, 64, 65, 256, 257):
        out.append((f"fresh {cap}", cap, pairs_fresh(cap)))            # n_flows == flow_cap
    out.append(("fresh 200 of 257", 257, pairs_fresh(200)))            # n_flows < flow_cap, ending inside a wave
    for how in ("role0", "role1", "alternating"):
        out.append((f"hub {how}", 1030, pairs_hub(1030, how)))
    out.append(("3 hosts", 1100, pairs_pool(1030, 3, 5, mixed=False)))
    out.append(("mixed 50", 700, pairs_pool(600, 50, 6)))
    out.append(("mixed pair", 8, [(v4(0x01020304), v4(0x01020304)), (v6(0x01020304 << 96), v6(1)), (v4(0x01020304), v4(9)),
                                  (v6(1), v6(0x01020304 << 96))]))
    return out
