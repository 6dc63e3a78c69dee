"""A packet's position inside its flow and the per-flow cut-off, restated as a plain loop over the
packets in order (bt_flow_seq_*, include/beatrice_gpu.h): flow numbers come from the caller, lengths
from the descriptors, the selection from verdict-layout words. Nothing here calls the code under test."""
import numpy as np

import flowtcp_ref as tr

U64 = (1 << 64) - 1
KEEP_UNKEYED = 1
SEQ_NONE = 0xFFFFFFFF
SEQ_MAX = 0xFFFFFFFE
OFF_NONE = U64
SENTINELS = frozenset(tr.SENTINELS)

SEQ_REC = np.dtype({"names": ["packets", "bytes"], "formats": ["<u8", "<u8"], "offsets": [0, 8], "itemsize": 16})


def number(table: np.ndarray, flow_id, lens, select, max_packets: int = 0, max_bytes: int = 0, flags: int = 0):
    """One batch numbered against `table` (SEQ_REC, in place). select: verdict-layout words or None
    (every packet); lens: frame lengths. Returns (seq u32 [n], byte_off u64 [n], out_select words,
    the result dict) of bt_flow_seq_*."""
    ids = [int(x) for x in np.asarray(flow_id, np.uint32)]
    ln = [min(int(x), 65535) for x in lens]
    n, cap = len(ids), len(table)
    words = None if select is None else [int(w) for w in select]
    seq, off = [SEQ_NONE] * n, [OFF_NONE] * n
    out = [0] * ((n + 63) // 64)
    state = {}        # flow -> [packets, bytes], the flows this call numbers
    res = dict.fromkeys(("selected", "numbered", "unkeyed", "bad_ids", "kept", "flows", "new_flows", "numbered_bytes", "kept_bytes"), 0)
    for i in range(n):
        if words is not None and not (words[i >> 6] >> (i & 63)) & 1:
            continue
        res["selected"] += 1
        f = ids[i]
        if f >= cap:
            if f in SENTINELS:
                res["unkeyed"] += 1
                if flags & KEEP_UNKEYED:
                    out[i >> 6] |= 1 << (i & 63)
                    res["kept"] += 1
            else:
                res["bad_ids"] += 1
            continue
        if f not in state:
            state[f] = [int(table["packets"][f]), int(table["bytes"][f])]
            res["flows"] += 1
            res["new_flows"] += state[f][0] == 0
        pk, by = state[f]
        seq[i], off[i] = min(pk, SEQ_MAX), by
        if (max_packets == 0 or pk < max_packets) and (max_bytes == 0 or by < max_bytes):
            out[i >> 6] |= 1 << (i & 63)
            res["kept"] += 1
            res["kept_bytes"] += ln[i]
        state[f] = [(pk + 1) & U64, (by + ln[i]) & U64]
        res["numbered"] += 1
        res["numbered_bytes"] += ln[i]
    for f, (pk, by) in state.items():
        table["packets"][f], table["bytes"][f] = pk, by
    res = {"n": n, **res, "reserved": [0, 0]}
    order = ("n", "selected", "numbered", "unkeyed", "bad_ids", "kept", "flows", "new_flows", "numbered_bytes", "kept_bytes", "reserved")
    return (np.array(seq, np.uint32), np.array(off, np.uint64), np.array(out, np.uint64), {k: res[k] for k in order})
