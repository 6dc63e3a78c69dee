"""CPU: bt_tally (include/beatrice_gpu.h) as the ctypes binding lays it out, and the refusals of
bt_tally_device that need no GPU."""
import ctypes
import os
import re

from beatrice_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BT_E_INVALID_ARGUMENT = 1
SIZES = {"uint64_t": 8, "uint32_t": 4}


def _header_fields():
    """(name, offset, bytes) of every field of bt_tally, from the header's own declaration
    (natural alignment, as the C compiler lays out uint32_t / uint64_t members)."""
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    body = re.search(r"typedef struct bt_tally \{(.*?)\} bt_tally;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        size = SIZES[ctype]
        for name in names.split(","):
            dims = [int(d) for d in re.findall(r"\[(\d+)\]", name)]
            count = 1
            for d in dims:
                count *= d
            off = (off + size - 1) // size * size
            fields.append((re.sub(r"\[.*", "", name).strip(), off, size * count))
            off += size * count
    return fields, off


def test_tally_struct_matches_the_header():
    fields, total = _header_fields()
    assert total == 2304 == ctypes.sizeof(abi.Tally)
    assert [f[0] for f in fields] == [name for name, _ in abi.Tally._fields_]
    for name, off, size in fields:
        f = getattr(abi.Tally, name)
        assert (f.offset, f.size) == (off, size), name
    assert abi.Tally.code.offset == 40 and abi.Tally.slot.offset == 72 and abi.Tally.bytes.offset == 2120
    assert abi.Tally.layer_present.offset == 2152 and abi.Tally.reserved.offset == 2280
    assert (abi.TALLY_STOP_AT_THROW, abi.TALLY_ACCUMULATE) == (1, 2)
    src = open(os.path.join(ROOT, "include", "beatrice_gpu.h")).read()
    assert re.search(r"#define BT_TALLY_STOP_AT_THROW 0x1u", src) and re.search(r"#define BT_TALLY_ACCUMULATE\s+0x2u", src)


def test_tally_as_dict_round_trip():
    t = abi.Tally()
    t.n, t.first_host_slot = 7, 5
    t.slot[1][63] = 1 << 40
    t.layer_ok[7] = 9
    t2 = abi.Tally.from_bytes(bytes(t))
    d = t2.as_dict()
    assert d["n"] == 7 and d["first_host_slot"] == 5 and d["slot"][1][63] == 1 << 40 and d["layer_ok"][7] == 9
    assert len(d["slot"]) == 4 and len(d["slot"][0]) == 64 and d["reserved"] == [0, 0, 0]


def test_tally_device_refuses_a_null_context_without_a_gpu():
    out = abi.Tally()
    before = bytes(out)
    dec = (ctypes.c_uint8 * 16)()
    L = abi.lib()
    assert "bt_tally_device" in abi.EXPORTS
    assert L.bt_tally_device(None, dec, 16, None, None, 0, 0, ctypes.byref(out), None) == BT_E_INVALID_ARGUMENT
    assert L.bt_tally_device(None, None, 0, None, None, 0, 0, None, None) == BT_E_INVALID_ARGUMENT
    assert bytes(out) == before
    assert b"null context" in L.bt_last_error()
