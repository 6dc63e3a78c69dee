"""CPU: bt_pcap_index (beatrice_amd/csrc/bt_pcap.cpp), the host-only index of a classic pcap
file held in memory: one descriptor per whole record, in all four magics, up to the last whole
record of a truncated file; other link types and pcapng refused."""
import struct

import numpy as np
import pytest

import pcap_util as pu
from beatrice_amd import abi

BT_E_INVALID_ARGUMENT, BT_E_NOT_IMPLEMENTED = 1, 11
FRAMES = [bytes([k & 0xFF]) * ln for k, ln in enumerate([60, 0, 1, 1514, 61, 9000, 64])]


def _expected_desc(frames):
    """Offsets of the records' data: 24-B global header, 16-B record headers."""
    out, pos = [], 24
    for f in frames:
        out.append((pos + 16) | (len(f) << 48))
        pos += 16 + len(f)
    return np.array(out, np.uint64), pos


@pytest.mark.parametrize("nanosecond", [False, True])
@pytest.mark.parametrize("swapped", [False, True])
def test_four_magics(nanosecond, swapped):
    buf = pu.build(FRAMES, nanosecond=nanosecond, swapped=swapped)
    want, end = _expected_desc(FRAMES)
    assert end == len(buf)
    info, desc = abi.pcap_index(buf)
    assert np.array_equal(desc, want)
    assert info == {"magic": pu.MAGIC_NSEC if nanosecond else pu.MAGIC_USEC, "swapped": int(swapped),
                    "nanosecond": int(nanosecond), "snaplen": 65535, "linktype": 1, "truncated": 0, "end": end}
    # the first four bytes on disk: the magic in the writer's byte order
    assert buf[:4] == struct.pack(">I" if swapped else "<I", info["magic"])


def test_zero_records():
    info, desc = abi.pcap_index(pu.global_header())
    assert len(desc) == 0 and info["end"] == 24 and info["truncated"] == 0
    assert abi.pcap_index(pu.global_header(), count_only=True)[1] == 0


@pytest.mark.parametrize("swapped", [False, True])
def test_truncated_tails(swapped):
    buf = pu.build(FRAMES, swapped=swapped)
    want, end = _expected_desc(FRAMES)
    last = end - 16 - len(FRAMES[-1])          # where the last record's header starts
    for cut, n in [(last + 1, 6), (last + 15, 6),          # inside the last record's header
                   (last + 16, 6), (last + 16 + 63, 6),    # inside its data (64 B)
                   (24 + 7, 0), (24 + 16 + 59, 0)]:        # inside the first record
        info, desc = abi.pcap_index(buf[:cut])
        assert info["truncated"] == 1, cut
        assert np.array_equal(desc, want[:n]), cut
        assert info["end"] == (last if n == 6 else 24), cut
    # a cut exactly between two records is a whole, shorter file
    info, desc = abi.pcap_index(buf[:last])
    assert info["truncated"] == 0 and len(desc) == 6 and info["end"] == last


def test_other_link_types_and_pcapng_are_not_implemented():
    for swapped in (False, True):
        buf = pu.global_header(linktype=113, swapped=swapped) + pu.record(b"x" * 60, 0, swapped)
        with pytest.raises(abi.BtError) as e:
            abi.pcap_index(buf)
        assert e.value.code == BT_E_NOT_IMPLEMENTED and "113" in str(e.value)
    pcapng = struct.pack("<III", 0x0A0D0D0A, 28, 0x1A2B3C4D) + bytes(16)
    with pytest.raises(abi.BtError) as e:
        abi.pcap_index(pcapng)
    assert e.value.code == BT_E_NOT_IMPLEMENTED


def test_invalid_files_are_refused():
    for buf in (b"", b"\xd4\xc3\xb2\xa1" + bytes(19), b"\x00" * 24, b"PCAP" + bytes(40)):
        with pytest.raises(abi.BtError) as e:
            abi.pcap_index(buf)
        assert e.value.code == BT_E_INVALID_ARGUMENT, buf[:8]
    info = abi.PcapInfo()
    n = abi.ctypes.c_uint64(0)
    a = np.frombuffer(pu.global_header(), np.uint8)
    L = abi.lib()
    assert L.bt_pcap_index(None, 24, abi.ctypes.byref(info), None, 0, abi.ctypes.byref(n)) == BT_E_INVALID_ARGUMENT
    assert L.bt_pcap_index(a.ctypes.data, 24, None, None, 0, abi.ctypes.byref(n)) == BT_E_INVALID_ARGUMENT
    assert L.bt_pcap_index(a.ctypes.data, 24, abi.ctypes.byref(info), None, 0, None) == BT_E_INVALID_ARGUMENT


@pytest.mark.parametrize("swapped", [False, True])
def test_incl_len_limit(swapped):
    e = ">" if swapped else "<"
    big = bytes(65535)
    buf = pu.global_header(swapped=swapped) + pu.record(b"ab", 0, swapped) + pu.record(big, 1, swapped)
    info, desc = abi.pcap_index(buf)
    assert [int(d) >> 48 for d in desc] == [2, 65535] and info["truncated"] == 0
    over = pu.global_header(swapped=swapped) + pu.record(b"ab", 0, swapped) + \
        struct.pack(e + "IIII", 1, 2, 65536, 65536) + bytes(65536)
    with pytest.raises(abi.BtError) as err:
        abi.pcap_index(over)
    assert err.value.code == BT_E_INVALID_ARGUMENT and "65536" in str(err.value)


def test_count_only_and_short_descriptor_array():
    buf = pu.build(FRAMES)
    want, end = _expected_desc(FRAMES)
    info, n = abi.pcap_index(buf, count_only=True)
    assert n == len(FRAMES) and info["end"] == end
    # a descriptor array shorter than the file: the first `cap` entries, the full count
    a = np.frombuffer(buf, np.uint8)
    desc = np.full(5, 0xA5A5A5A5A5A5A5A5, np.uint64)
    cnt = abi.ctypes.c_uint64(0)
    pi = abi.PcapInfo()
    assert abi.lib().bt_pcap_index(a.ctypes.data, len(a), abi.ctypes.byref(pi), desc.ctypes.data, 3,
                                   abi.ctypes.byref(cnt)) == 0
    assert cnt.value == len(FRAMES) and np.array_equal(desc[:3], want[:3])
    assert (desc[3:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
