"""The fan-out's expected values, restated in numpy / Python and independent of the code under
test: a bit-serial Toeplitz hash, the flow-key rule of include/beatrice_gpu.h applied to a bt_rec,
a Python walk of DESIGN.md §2 for frames that have no golden record, and the stable K-way
partition (queue bytes, idx, select_q rows, bt_fanout_result)."""
import numpy as np

DEFAULT_KEY = bytes.fromhex("6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c6a42b73bbeac01fa")
SYMMETRIC_KEY = bytes.fromhex("6d5a") * 20
NONE, V4, V4_L4, V6, V6_L4 = range(5)
L_IPV4, L_IPV6, L_TCP, L_UDP = 0x08, 0x10, 0x20, 0x40
MASK48 = np.uint64((1 << 48) - 1)


def toeplitz(key: bytes, data: bytes) -> int:
    """RSS Toeplitz, MSB first: every set input bit i XORs in the 32 key bits from bit i on."""
    k = int.from_bytes(key, "big")
    kbits = len(key) * 8
    h = 0
    for i in range(len(data) * 8):
        if data[i >> 3] & (0x80 >> (i & 7)):
            h ^= (k >> (kbits - 32 - i)) & 0xFFFFFFFF
    return h


def toeplitz_many(key: bytes, inputs: np.ndarray, nbytes: np.ndarray) -> np.ndarray:
    """toeplitz() of inputs[i, :nbytes[i]] for every row (inputs: [n, 36] uint8)."""
    k = int.from_bytes(key, "big")
    kbits = len(key) * 8
    h = np.zeros(len(inputs), np.uint32)
    for i in range(36 * 8):
        bit = (inputs[:, i >> 3] & (0x80 >> (i & 7))) != 0
        bit &= (i >> 3) < nbytes
        h ^= np.where(bit, np.uint32((k >> (kbits - 32 - i)) & 0xFFFFFFFF), np.uint32(0))
    return h


def key_of_rec(rec: np.ndarray, l3_only: bool = False):
    """The flow key of bt_rec rows ([n, 96] uint8): (inputs [n, 36], nbytes [n], klass [n])."""
    rec = np.ascontiguousarray(rec).reshape(-1, 96)
    n = len(rec)
    ok = rec[:, 25]
    inputs = np.zeros((n, 36), np.uint8)
    nbytes = np.zeros(n, np.int64)
    klass = np.zeros(n, np.int64)
    ports = np.stack([rec[:, 69], rec[:, 68], rec[:, 71], rec[:, 70]], axis=1)   # u16 LE fields in wire order
    l4 = ((ok & (L_TCP | L_UDP)) != 0) & (not l3_only)
    v4 = (ok & L_IPV4) != 0
    flags = rec[:, 38].astype(np.int64) | (rec[:, 39].astype(np.int64) << 8)
    v4l4 = v4 & l4 & ((flags & 0x3FFF) == 0)
    inputs[v4, 0:8] = rec[v4, 44:52]
    inputs[v4l4, 8:12] = ports[v4l4]
    nbytes[v4], klass[v4] = 8, V4
    nbytes[v4l4], klass[v4l4] = 12, V4_L4
    v6 = ((ok & L_IPV6) != 0) & ~v4
    v6l4 = v6 & l4
    inputs[v6, 0:32] = rec[v6, 36:68]
    inputs[v6l4, 32:36] = ports[v6l4]
    nbytes[v6], klass[v6] = 32, V6
    nbytes[v6l4], klass[v6l4] = 36, V6_L4
    return inputs, nbytes, klass


def walk(frame: bytes, l3_only: bool = False):
    """DESIGN.md §2's layer walk over one frame, as far as the flow key needs it: (key bytes, class)."""
    n = len(frame)
    be16 = lambda o: (frame[o] << 8) | frame[o + 1]  # noqa: E731
    if n < 14:
        return b"", NONE
    et, k = be16(12), 0
    while k < 2 and et in (0x8100, 0x88A8):
        vo = 12 + 4 * k
        if n - vo < 4 or n < vo + 6:
            return b"", NONE
        et = be16(vo + 4)
        k += 1
    o3 = 14 + 4 * k
    if et == 0x0800:
        if n - o3 < 20:
            return b"", NONE
        addr = frame[o3 + 12:o3 + 20]
        o4, proto = o3 + 4 * (frame[o3] & 0xF), frame[o3 + 9]
        need = {6: 20, 17: 8}.get(proto, 0)
        if l3_only or not need or o4 > n or n - o4 < need or (be16(o3 + 6) & 0x3FFF):
            return bytes(addr), V4
        return bytes(addr + frame[o4:o4 + 4]), V4_L4
    if et == 0x86DD:
        if n - o3 < 40:
            return b"", NONE
        addr = frame[o3 + 8:o3 + 40]
        o4, need = o3 + 40, {6: 20, 17: 8}.get(frame[o3 + 6], 0)
        if l3_only or not need or n - o4 < need:
            return bytes(addr), V6
        return bytes(addr + frame[o4:o4 + 4]), V6_L4
    return b"", NONE


def key_of_frames(frames, l3_only: bool = False):
    """key_of_rec's triple from walk() over a list of frames."""
    inputs = np.zeros((len(frames), 36), np.uint8)
    nbytes = np.zeros(len(frames), np.int64)
    klass = np.zeros(len(frames), np.int64)
    for i, f in enumerate(frames):
        kb, klass[i] = walk(bytes(f), l3_only)
        inputs[i, :len(kb)] = np.frombuffer(kb, np.uint8)
        nbytes[i] = len(kb)
    return inputs, nbytes, klass


def default_reta(queues: int) -> np.ndarray:
    return (np.arange(128) % queues).astype(np.uint8)


def select_bits(select, n: int) -> np.ndarray:
    """The n selection bits of verdict-layout words (None: all ones); bits at or above n are dropped."""
    if select is None:
        return np.ones(n, bool)
    w = np.ascontiguousarray(select, np.uint64)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """Verdict-layout words of a bool array (bits past its end are 0)."""
    n = len(bits)
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


def expected(hashes: np.ndarray, klass: np.ndarray, lens: np.ndarray, queues: int, reta=None, select=None) -> dict:
    """Every output of bt_flow_fanout_device for n packets with these hashes, classes and frame lengths."""
    n = len(hashes)
    reta = default_reta(queues) if reta is None else np.asarray(reta, np.uint8)
    sel = select_bits(select, n)
    q_all = reta[hashes & 127] if n else np.zeros(0, np.uint8)
    queue = np.where(sel, q_all, 0xFF).astype(np.uint8)
    ntiles = (n + 63) // 64
    idx_parts, start, nbytes, rows = [], [0], [0] * 64, np.zeros((queues, ntiles), np.uint64)
    lens = np.minimum(np.asarray(lens, np.int64), 65535)
    for q in range(queues):
        mine = queue == q
        idx_parts.append(np.nonzero(mine)[0])
        start.append(start[-1] + int(mine.sum()))
        nbytes[q] = int(lens[mine].sum())
        if ntiles:
            rows[q] = pack_bits(mine)
    start += [start[-1]] * (65 - len(start))
    res = {"n": n, "n_selected": int(sel.sum()), "start": start, "pad0": 0, "bytes": nbytes,
           "klass": [int((klass[sel] == k).sum()) for k in range(5)], "pad1": 0}
    idx = np.concatenate(idx_parts).astype(np.uint32) if idx_parts else np.zeros(0, np.uint32)
    return {"hash": hashes.astype(np.uint32), "queue": queue, "idx": idx, "select_q": rows.reshape(-1), "result": res}
