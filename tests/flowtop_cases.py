"""Crafted tracker states for the top-K tests (CPU and GPU): a header and records built here, value
patterns at which each part of the selection can go wrong, and the list of k for a table size.
Nothing here calls the code under test."""
import struct

import numpy as np

import flowtcp_ref as tr
import flowtop_ref as top
import flowtrack_ref as fkr

N_FLOWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000]
U64 = np.uint64


def caps(n_flows: int):
    """flow_cap == n_flows (at least 1) and flow_cap > n_flows, ending inside a block."""
    return sorted({max(1, n_flows), n_flows + 37})


def ks(n_flows: int):
    """The issue's k, and two that end among the ties in the middle of a block."""
    out = [0, 1, 2, n_flows - 1, n_flows, n_flows + 1, 4096]
    if n_flows >= 1023:
        out += [300, 600]
    return sorted({k for k in out if 0 <= k <= top.MAX_K})


def header(flags: int, flow_cap: int, slots: int, n_flows: int, seq: int = 3) -> bytes:
    """A bt_flow_track_hdr (128 B)."""
    return struct.pack("<6I", fkr.MAGIC, flags, flow_cap, slots, n_flows, seq) + bytes(104)


def garbage(recs: np.ndarray, tcp: np.ndarray, n_flows: int):
    """Records at or past n_flows: large values in every field a metric reads. They must not be selected."""
    tail = np.arange(len(recs) - n_flows, dtype=U64)
    recs["bytes"][n_flows:, 0] = U64(0xFFFFFFFFFFFFFF00) - tail
    recs["packets"][n_flows:, 1] = U64(0xFFFFFFFFFFFFFFFF) - tail
    recs["last_ts"][n_flows:] = U64(0xFFFFFFFFFFFFFFF0)
    recs["key"][n_flows:, 0] = 0xEE
    tcp["syn_packets"][n_flows:] = 0xFFFFFFF0
    tcp["rst_packets"][n_flows:] = 0xFFFFFFFF


def patterns(n_flows: int, flow_cap: int, seed: int = 0):
    """[(name, metrics, records [flow_cap], side table [flow_cap])]: every record carries its flow
    number in its key, so that a gathered record shows where it came from."""
    rng = np.random.default_rng(1000 * n_flows + flow_cap + seed)
    i = np.arange(n_flows, dtype=U64)
    out = []

    def case(name, metrics, fill):
        recs, tcp = np.zeros(flow_cap, fkr.FLOW_TRACK_REC), np.zeros(flow_cap, tr.TCP_REC)
        recs["key"][:, :4] = np.arange(flow_cap, dtype="<u4").view(np.uint8).reshape(-1, 4)
        recs["klass"] = 1
        live, side = recs[:n_flows], tcp[:n_flows]
        fill(live, side)
        garbage(recs, tcp, n_flows)
        out.append((name, metrics, recs, tcp))

    def equal(r, t):
        r["bytes"][:, 0], r["bytes"][:, 1] = 600, 400
        r["packets"][:, 0] = 0          # zero-valued flows rank like any other
        t["syn_packets"] = 2
    case("equal", (top.BYTES, top.PACKETS, top.TCP_SYN), equal)

    def two(r, t):
        # a few large flows; the many small ones tie at the threshold across every block boundary
        r["bytes"][:, 0] = np.where((i % U64(293)) == U64(3), U64(90000), U64(50))
        r["packets"][:, 1] = np.where((i % U64(2)) == U64(1), U64(9), U64(4))
        t["rst_packets"] = np.where(i >= U64(n_flows // 2), 1, 0)
    case("two values", (top.BYTES, top.PACKETS, top.TCP_RST), two)

    def low(r, t):
        r["bytes"][:, 1] = U64(0x0102030405060700) + (i * U64(37)) % U64(256)
    case("lowest byte", (top.BYTES,), low)

    def high(r, t):
        r["packets"][:, 0] = ((i * U64(73)) % U64(256)) << U64(56) | U64(5)     # 0x80.. and above: >= 2^63
    case("highest byte", (top.PACKETS,), high)

    def wrap(r, t):
        r["bytes"][:, 0] = U64(0xFFFFFFFFFFFFFFFF) - (i % U64(7))
        r["bytes"][:, 1] = i * U64(3) + U64(10)                                  # the sum wraps past 2^64
    case("wrap", (top.BYTES,), wrap)

    def full(r, t):
        r["bytes"][:, 0] = rng.integers(0, 1 << 64, n_flows, dtype=U64)
        r["packets"][:, 0] = rng.integers(0, 1 << 63, n_flows, dtype=U64)
        r["packets"][:, 1] = rng.integers(0, 1 << 63, n_flows, dtype=U64)
        r["first_ts"] = rng.integers(0, 1000, n_flows, dtype=U64)
        r["last_ts"] = rng.integers(0, 1000, n_flows, dtype=U64)              # about half run backwards: 0
        t["flags"][:, 0] = rng.integers(0, 256, n_flows)
        t["syn_packets"] = rng.integers(0, 4, n_flows)
        t["fin_packets"] = rng.integers(0, 1 << 32, n_flows, dtype=U64)
        t["rst_packets"] = rng.integers(0, 1 << 32, n_flows, dtype=U64)
    case("random", top.METRICS, full)
    return out
