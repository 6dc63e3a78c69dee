"""The top-K query's expected values, restated in numpy / Python and independent of the code under
test: the value of every flow from its record's fields (or its side record's), the order (value
descending, flow number ascending) by np.lexsort over the values' split u32 halves, so that values
at and above 2^63 order correctly, and the result's counts and sums as Python ints mod 2^64. Every
output of bt_flow_track_top_* comes out of expected()."""
import numpy as np

BYTES, PACKETS, DURATION, TCP_SYN, TCP_RST = range(5)
METRICS = (BYTES, PACKETS, DURATION, TCP_SYN, TCP_RST)
MAX_K = 4096
M64 = (1 << 64) - 1


def values(metric: int, recs: np.ndarray, tcp=None) -> np.ndarray:
    """The u64 value of every record (FLOW_TRACK_REC rows; tcp: TCP_REC rows beside them)."""
    if metric == BYTES:
        return recs["bytes"][:, 0] + recs["bytes"][:, 1]        # u64 arithmetic wraps mod 2^64
    if metric == PACKETS:
        return recs["packets"][:, 0] + recs["packets"][:, 1]
    if metric == DURATION:
        first, last = recs["first_ts"], recs["last_ts"]
        return np.where(last >= first, last - first, np.uint64(0)).astype(np.uint64)
    name = {TCP_SYN: "syn_packets", TCP_RST: "rst_packets"}[metric]
    return tcp[name][:len(recs)].astype(np.uint64)


def order(vals: np.ndarray) -> np.ndarray:
    """Every flow number in the top's order: value descending, then flow number ascending."""
    v = np.asarray(vals, np.uint64)
    hi, lo = (v >> np.uint64(32)).astype(np.int64), (v & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.lexsort((np.arange(len(v)), -lo, -hi)).astype(np.uint32)


def expected(metric: int, k: int, recs: np.ndarray, tcp=None) -> dict:
    """recs: the n_flows live records; tcp: at least n_flows side records or None."""
    with np.errstate(over="ignore"):
        v = values(metric, recs, tcp).astype(np.uint64)
    n = len(v)
    n_top = min(k, n)
    ids = order(v)[:n_top]
    top_value = v[ids]
    threshold = int(top_value[-1]) if n_top else 0
    res = {"n_flows": n, "n_top": n_top, "status": 0, "metric": metric,
           "n_ties": int((v == np.uint64(threshold)).sum()) if n_top else 0, "reserved": 0, "threshold": threshold,
           "total": sum(int(x) for x in v) & M64, "top_total": sum(int(x) for x in top_value) & M64}
    return {"top_id": ids, "top_value": top_value, "top": recs[ids], "top_tcp": None if tcp is None else tcp[ids], "result": res}
