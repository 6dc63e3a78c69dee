"""The per-flow mark side table and the selection built from it, restated in numpy
(bt_flow_mark_update_* / bt_flow_mark_select_*, include/beatrice_gpu.h): flow numbers come from
flowtab_ref / flowtrack_ref, lengths from the descriptors, hits from verdict-layout words. Nothing
here calls the code under test."""
import numpy as np

import flow_ref as fr
import flowtcp_ref as tr

U64 = (1 << 64) - 1
ALL_BITS = 1
SET, AND, OR, ANDNOT = range(4)

MARK_REC = np.dtype({
    "names": ["marks", "hit_packets", "hit_bytes", "first_hit_ts_c", "last_hit_ts"],
    "formats": ["<u4", "<u4", "<u8", "<u8", "<u8"],
    "offsets": [0, 4, 8, 16, 24],
    "itemsize": 32,
})
SENTINELS = np.array(tr.SENTINELS, np.uint32)


def update(table: np.ndarray, flow_id, lens, hit, mark: int, ts) -> dict:
    """One batch's hits added to `table` (MARK_REC, in place): the result dict of bt_flow_mark_update_*.
    hit: verdict-layout words or None (every packet); lens: frame lengths; ts: one stamp per packet,
    or a scalar for the whole batch."""
    flow_id = np.asarray(flow_id, np.uint32)
    n, cap = len(flow_id), len(table)
    ts = np.broadcast_to(np.asarray(ts, np.uint64), (n,))
    is_hit = fr.select_bits(hit, n).astype(bool) if n else np.zeros(0, bool)
    ok = is_hit & (flow_id < cap)
    unkeyed = is_hit & np.isin(flow_id, SENTINELS)
    f, t = flow_id[ok].astype(np.int64), ts[ok]
    lacked = (table["marks"] & np.uint32(mark)) != np.uint32(mark)
    touched = np.zeros(cap, bool)
    touched[f] = True
    np.bitwise_or.at(table["marks"], f, np.uint32(mark))
    np.add.at(table["hit_packets"], f, np.uint32(1))                                       # mod 2^32
    np.add.at(table["hit_bytes"], f, np.minimum(np.asarray(lens, np.int64)[ok], 65535).astype(np.uint64))   # mod 2^64
    np.maximum.at(table["first_hit_ts_c"], f, ~t)
    np.maximum.at(table["last_hit_ts"], f, t)
    return {"n": n, "hit_packets": int(is_hit.sum()), "marked_packets": int(ok.sum()), "unkeyed_hits": int(unkeyed.sum()),
            "bad_ids": int((is_hit & ~ok & ~unkeyed).sum()), "new_marked_flows": int((lacked & touched).sum()), "reserved": [0, 0]}


def select(table: np.ndarray, flow_id, mask: int, op: int = SET, flags: int = 0, base=None):
    """(out words, result dict) of bt_flow_mark_select_*."""
    flow_id = np.asarray(flow_id, np.uint32)
    n, cap = len(flow_id), len(table)
    keyed = flow_id < cap
    got = np.zeros(n, np.uint32)
    got[keyed] = table["marks"][flow_id[keyed].astype(np.int64)] & np.uint32(mask)
    m = (got == np.uint32(mask)) if flags & ALL_BITS else (got != 0)
    b = fr.select_bits(base, n).astype(bool) if (base is not None and n) else np.zeros(n, bool)
    out = m if op == SET else (b & m) if op == AND else (b | m) if op == OR else (b & ~m)
    return fr.pack_bits(out), {"n": n, "n_marked": int(m.sum()), "n_out": int(out.sum()),
                           "bad_ids": int((~keyed & ~np.isin(flow_id, SENTINELS)).sum()), "reserved": [0, 0, 0, 0]}
