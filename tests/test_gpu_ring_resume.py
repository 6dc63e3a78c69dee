"""GPU: the ring stage's two-pass PAYLOAD path (bt_ring_stage_tpv3_ex, BT_RING_RESUME_PAYLOAD).
Gathered batches hold frame bytes 12..43 only, so their launch leaves DECIDE_HOST at a GPU PAYLOAD
slot; with the flag the resume kernel follows each gathered batch over the frames in the ring, and
every mode decides as the in-place run of the same ring (and the compiled reference where built)."""
import numpy as np
import pytest

import oracle_lib as ol
from beatrice_amd import abi, synth
from golden_util import compare_decisions

pytestmark = pytest.mark.gpu

N = 20_000
PROGRAM = [{"type": abi.PROTOCOL, "expr": "udp", "priority": 3},
           {"type": abi.PAYLOAD, "expr": "[\\x80-\\xff]{3}|\\d\\d", "priority": 2},
           {"type": abi.PORT_RANGE, "expr": "0-40000", "priority": 1}]
MODES = {"in_place": {}, "lean_mix": dict(gather=True, in_place_every=2), "lean_all": dict(gather=True),
         "lean_split": dict(gather=True, in_place_blocks=3), "adaptive": dict(gather="adaptive")}


def _stage(ctx, ring, used, register_ring_desc=True, with_ring_desc=True, **kw):
    """The ring stage over a ring image, every buffer registered on pages of its own. Returns a
    dict of the call's results (copies)."""
    ring = abi.host_copy(ring)
    desc = abi.host_array(N + 64, np.uint64)
    dec = abi.host_array(N + 64)
    ver = abi.host_array((N + 127) // 64, np.uint64)
    slots = abi.host_array((N + 64) * abi.PREFIX_SLOT) if kw.get("gather") else None
    rdesc = abi.host_array(N + 64, np.uint64) if with_ring_desc else None
    held = [a for a in (ring, desc, dec, ver, slots, rdesc if register_ring_desc else None) if a is not None]
    for a in held:
        ctx.register(a)
    try:
        res = abi.ring_stage_tpv3(ctx, ring, synth.TPV3_BLOCK, used, desc, dec, ver, slots, batch_blocks=7,
                                  ring_desc=rdesc, **kw)
    finally:
        for a in held:
            ctx.unregister(a)
    got = res[0]
    return {"n": got, "n_pass": res[1], "n_host": res[2] if len(res) > 2 else None, "desc": desc[:got].copy(),
            "decide": dec[:got].copy(), "verdict": ver[:(got + 63) // 64].copy()}


@pytest.fixture(scope="module", params=[synth.C3, synth.FUZZ], ids=["c3", "fuzz"])
def ring_case(request, gpu_ctx):
    """A 20,000-frame ring and its in-place decisions under PROGRAM (one pass over whole frames)."""
    data, desc0 = synth.capture(request.param, N, seed=33)
    ring, rdesc, used = synth.tpv3_ring(data, desc0)
    assert len(rdesc) == N
    assert [abi.KINDS[s.kind] for s in gpu_ctx.compile(PROGRAM)] == ["PROTO_EQ", "PAYLOAD", "PORT"]
    ref = _stage(gpu_ctx, ring, used, with_ring_desc=False)
    assert ref["n"] == N and not ((ref["decide"] >> 6) == abi.DECIDE_HOST).any()
    codes = np.bincount(ref["decide"] >> 6, minlength=4)
    assert codes[abi.DECIDE_PASS] >= 10 and codes[abi.DECIDE_REJECT] >= 10
    assert (ref["decide"] == ((abi.DECIDE_REJECT << 6) | 1)).sum() >= 900     # the PAYLOAD slot's own rejections
    if ol.ref_available():
        code, src = ol.ref_filter(ring, rdesc, N, PROGRAM)
        compare_decisions(ref["decide"], code, src, PROGRAM, where="ring in place")
    return ring, rdesc, used, ref


@pytest.mark.parametrize("mode", list(MODES))
def test_resumed_modes_decide_as_in_place(gpu_ctx, ring_case, mode):
    ring, rdesc, used, ref = ring_case
    gpu_ctx.compile(PROGRAM)
    got = _stage(gpu_ctx, ring, used, resume_payload=True, want_host=True, **MODES[mode])
    assert got["n"] == N
    bad = np.nonzero(got["decide"] != ref["decide"])[0]
    assert len(bad) == 0, f"{mode}: {len(bad)} decisions differ from in place, first {bad[:5]}"
    want = (got["decide"] >> 6) == abi.DECIDE_PASS
    bits = np.unpackbits(got["verdict"].view(np.uint8), bitorder="little")[:N].astype(bool)
    assert np.array_equal(bits, want)
    assert got["n_pass"] == int(want.sum()) == ref["n_pass"]
    assert got["n_host"] == 0


def test_without_the_flag_nothing_changes(gpu_ctx, ring_case):
    """flags = 0 through the new entry point equals bt_ring_stage_tpv3: the gathered batches
    keep DECIDE_HOST at the PAYLOAD slot and count as not passed."""
    ring, rdesc, used, ref = ring_case
    gpu_ctx.compile(PROGRAM)
    old = _stage(gpu_ctx, ring, used, with_ring_desc=False, gather=True)
    new = _stage(gpu_ctx, ring, used, want_host=True, gather=True)
    for k in ("n", "n_pass", "desc", "decide", "verdict"):
        assert np.array_equal(old[k], new[k]), k
    host = (old["decide"] >> 6) == abi.DECIDE_HOST
    assert host.any() and np.all((old["decide"] & 63)[host] == 1)
    assert new["n_host"] == int(host.sum())


def test_custom_slot_last_counts_host_frames(gpu_ctx, ring_case):
    ring, rdesc, used, ref = ring_case
    prog = PROGRAM + [{"type": abi.CUSTOM, "expr": "", "priority": 0, "custom": 1}]
    try:
        assert [abi.KINDS[s.kind] for s in gpu_ctx.compile(prog)] == ["PROTO_EQ", "PAYLOAD", "PORT", "HOST"]
        got = _stage(gpu_ctx, ring, used, resume_payload=True, want_host=True, gather=True)
    finally:
        gpu_ctx.compile(PROGRAM)
    host = (got["decide"] >> 6) == abi.DECIDE_HOST
    assert got["n_host"] == int(host.sum()) > 0 and np.all((got["decide"] & 63)[host] == 3)
    # the frames PROGRAM passes are the ones handed to the CUSTOM slot; the rest decide as before
    assert np.array_equal(host, (ref["decide"] >> 6) == abi.DECIDE_PASS)
    assert np.array_equal(got["decide"][~host], ref["decide"][~host])
    assert got["n_pass"] == 0 and not got["verdict"].any()


def test_gather_with_the_flag_needs_a_registered_ring_desc(gpu_ctx, ring_case):
    ring, rdesc, used, ref = ring_case
    gpu_ctx.compile(PROGRAM)
    with pytest.raises(abi.BtError, match="ring_desc"):
        _stage(gpu_ctx, ring, used, with_ring_desc=False, resume_payload=True, gather=True)
    with pytest.raises(abi.BtError, match="registered"):
        _stage(gpu_ctx, ring, used, register_ring_desc=False, resume_payload=True, gather=True)
