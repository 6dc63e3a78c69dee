"""GPU: the second pass of the PAYLOAD filter (bt_filter_resume_device, bt_payload_resume.hip)
over the two batch forms tests/test_gpu_payload_resume.py does not run: xdp_desc descriptors and a
fixed stride. Both go through the device's one "packet i -> (offset, length)" (frame_at,
beatrice_amd/csrc/bt_frames.h)."""
import numpy as np
import pytest

from beatrice_amd import abi, synth
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _single(ctx, data, desc, n, stride=0):
    run = abi.DeviceRun(ctx, data, desc, n, stride=stride, records=False)
    run.run()
    out = run.fetch()
    run.free()
    return out


def _two_pass(ctx, data, desc, n, stride=0, desc_format=abi.DESC_PACKED):
    """(first-pass decision bytes, outputs after the resume pass) of one batch (desc None: fixed
    stride): the first pass with BATCH_PREFIXES over the whole-frame data (the flag alone keeps the
    payload unread), the resume pass over the same batch with flags 0. The verdict words are
    overwritten in between, so every word read afterwards was rebuilt by the resume pass."""
    run = abi.DeviceRun(ctx, data, desc, n, stride=stride, records=False)
    try:
        run.batch.desc_format = desc_format
        run.batch.flags = abi.BATCH_PREFIXES
        run.run()
        first = run.fetch()["decide"].copy()
        run.batch.flags = 0
        run.d_ver.upload(np.full(run.d_ver.nbytes, 0xA5, np.uint8))
        ctx.resume_device(run.batch, run.outs)
        out = run.fetch()
    finally:
        run.free()
    return first, out


def _check_outputs(out, n):
    """Verdict words and the pass list against the decision bytes."""
    want = (out["decide"] >> 6) == abi.DECIDE_PASS
    bits = np.unpackbits(out["verdict"].view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:n].astype(bool), want) and not bits[n:].any()
    assert out["n_pass"] == int(want.sum())
    assert np.array_equal(out["pass_idx"], np.nonzero(want)[0])


def test_xdp_descriptors(gpu_ctx):
    """The same frames through {u64 addr; u32 len; u32 options} descriptors decide as through
    packed ones."""
    g, man = load_golden("http")
    n = len(g["desc"])
    gpu_ctx.compile(man["filter_sets"]["payload_chain"])
    xdp = np.zeros((n, 2), np.uint64)
    xdp[:, 0] = synth.desc_off(g["desc"]).astype(np.uint64)
    xdp[:, 1] = synth.desc_len(g["desc"]).astype(np.uint64)
    first, out = _two_pass(gpu_ctx, g["data"], xdp, n, desc_format=abi.DESC_XDP)
    first_p, packed = _two_pass(gpu_ctx, g["data"], g["desc"], n)
    assert np.array_equal(first, first_p) and ((first >> 6) == abi.DECIDE_HOST).any()
    assert np.array_equal(out["decide"], packed["decide"])
    assert np.array_equal(out["verdict"], packed["verdict"])
    assert out["n_pass"] == packed["n_pass"] == 192 and np.array_equal(out["pass_idx"], packed["pass_idx"])
    _check_outputs(out, n)


def test_fixed_stride(gpu_ctx):
    """A full tile, a partial tile and the boundary between tiles, 256-B frames built as
    tests/test_gpu_payload.py's test_fixed_stride_payload builds them, decided as the single
    whole-frame pass decides the same batch."""
    stride, n = 256, 64 * 3 + 17
    rng = np.random.default_rng(stride)
    frames = []
    for i in range(n):
        f = bytearray(rng.integers(0, 256, stride, dtype=np.uint8).tobytes())
        f[12:14] = b"\x08\x00" if i % 11 else b"\x86\xdd"
        ihl = 5 + (i % 7 == 0) * (i % 5)
        f[14] = 0x40 | ihl
        po = 14 + 4 * ihl
        w = (b"GET", b"POST", b"GE", b"xPOSTx")[i % 4]
        at = po + (i * 7) % max(1, stride - po - len(w) + 1)
        if i % 3 and at + len(w) <= stride:
            f[at:at + len(w)] = w
        frames.append(bytes(f))
    data, desc = synth.pack_frames(frames, align=stride)
    assert np.all(synth.desc_off(desc) == np.arange(n) * stride)
    data = data[: n * stride]
    f = [{"type": abi.PAYLOAD, "expr": "GET|POST", "priority": 1}]
    assert [abi.KINDS[s.kind] for s in gpu_ctx.compile(f)] == ["PAYLOAD"]
    first, out = _two_pass(gpu_ctx, data, None, n, stride=stride)
    assert np.all(first == ((abi.DECIDE_HOST << 6) | 0))
    single = _single(gpu_ctx, data, None, n, stride=stride)
    bad = np.nonzero(out["decide"] != single["decide"])[0]
    assert len(bad) == 0, f"{len(bad)} differ from the single pass, first {bad[:5]}"
    assert np.array_equal(out["verdict"], single["verdict"])
    codes = np.bincount(out["decide"] >> 6, minlength=4)
    assert codes[abi.DECIDE_PASS] >= 1 and codes[abi.DECIDE_REJECT] >= 1, codes
    assert codes[abi.DECIDE_PASS] + codes[abi.DECIDE_REJECT] == n
    _check_outputs(out, n)
