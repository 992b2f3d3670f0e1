"""The stream harness of tests/test_gpu_streams.py: runs one library call on a side stream behind a delayed producer and
compares every output, bit for bit, with the same call on the null stream.

The contract under test (include/mundy_hip.h): every entry point is ordered on the `stream` it is given, and everything
that does not return a host scalar is asynchronous.  A launch, memset or copy that lands on another stream runs BEFORE
the delayed producer has written the real inputs: it then sees the decoy (a valid problem of the same shapes) -- in the
inputs and, after one call on the decoy, in the library's own intermediates -- and computes the decoy's answer, which the
comparison catches.  Nothing is ever poisoned: a stray launch never reads garbage.

A case is a Case(...) below; run_on_side_stream(case, side, cycles_per_ms, synchronises) is the whole procedure.
"""
import struct
import time
from dataclasses import dataclass

import numpy as np
import torch

MIN_DELAY_MS, MAX_DELAY_MS, HOST_FACTOR = 30.0, 250.0, 10.0
SENTINEL = 0xA5  # byte pattern of the output buffers before the checked call

# ---- what the module measures (printed at the end, quoted in DESIGN.md) ----------------------------------------------
CALLED = set()          # library symbols fetched while a harness section was running (see recording_library)
_recording = [False]
REPORT = {"cycles_per_ms": None, "longest_delay_ms": 0.0, "cases": {}}


class _Recorder:
    """stands in for the loaded library: every attribute fetched while the harness runs is a called entry point"""

    def __init__(self, lib):
        object.__setattr__(self, "_lib", lib)

    def __getattr__(self, name):
        if _recording[0] and name.startswith("mhip_"):
            CALLED.add(name)
        return getattr(self._lib, name)


def recording_library(monkeypatch):
    """capi.load() -> a recorder around the loaded library (ops, pipeline and distributed reach the library through
    capi.load() alone: test_python_layers_reach_the_library_through_capi_load)"""
    from mundy_amd import capi
    rec = _Recorder(capi.load())
    monkeypatch.setattr(capi, "load", lambda: rec)
    return rec


class _Section:
    def __enter__(self):
        self.prev = _recording[0]
        _recording[0] = True

    def __exit__(self, *a):
        _recording[0] = self.prev


def recorded():
    return _Section()


class stop_on_device_fault:
    """a HIP error inside a test ends the session: nothing more is started on a device that has faulted"""

    def __enter__(self):
        return self

    def __exit__(self, kind, err, tb):
        if err is None or isinstance(err, AssertionError):
            return False
        from mundy_amd import capi
        text = str(err)
        # (capi.check raises MhipError for the HIP and no-device statuses only -- an argument or runtime status is a
        #  ValueError / RuntimeError and fails its one case; a library that was never built is not a device fault either)
        hip_status = isinstance(err, capi.MhipError) and "is missing" not in text
        if hip_status or "HIP error" in text or "hipError" in text or "illegal memory" in text:
            import pytest
            pytest.exit("device fault, session ended: %s" % text[:400], returncode=3)
        return False


# ---- delay -----------------------------------------------------------------------------------------------------------
def calibrate(side):
    """cycles of torch.cuda._sleep per millisecond on `side`, from one timed _sleep(10^7)"""
    with torch.cuda.stream(side):
        torch.cuda._sleep(1000)  # (the first launch of the kernel loads its code object)
        side.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(10 ** 7)
        b.record()
        side.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.05, "torch.cuda._sleep(10^7) took %g ms: no usable delay on this runtime" % ms
    REPORT["cycles_per_ms"] = 10 ** 7 / ms
    return REPORT["cycles_per_ms"]


def delay_ms_for(host_ms):
    return max(MIN_DELAY_MS, HOST_FACTOR * host_ms)


# ---- comparing outputs -------------------------------------------------------------------------------------------------
def _flatten(out, prefix=""):
    """outputs of a call -> {name: tensor | host scalar}; dicts, tuples and lists are walked, None dropped"""
    flat = {}
    if out is None:
        return flat
    if isinstance(out, dict):
        for k in out:
            flat.update(_flatten(out[k], "%s%s." % (prefix, k)))
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            flat.update(_flatten(v, "%s%d." % (prefix, i)))
    elif hasattr(out, "__dataclass_fields__"):
        for k in out.__dataclass_fields__:
            flat.update(_flatten(getattr(out, k), "%s%s." % (prefix, k)))
    else:
        flat[prefix.rstrip(".") or "out"] = out
    return flat


def _clone(flat):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in flat.items()}


def _bits(v):
    if isinstance(v, torch.Tensor):
        return v.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8).tobytes(), tuple(v.shape), str(v.dtype)
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, (bool, int, str, np.integer, np.bool_)):
        return int(v) if not isinstance(v, str) else v
    raise TypeError("output of type %s cannot be compared" % type(v))


def freeze(flat):
    return {k: _bits(v) for k, v in flat.items()}


def differing(a, b):
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    return sorted(k for k in a if a[k] != b[k])


def assert_same(got, ref, what):
    bad = differing(got, ref)
    assert not bad, "%s: outputs %s differ from the null-stream run (%d of %d)" % (what, bad, len(bad), len(ref))


# ---- the procedure -----------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """make(seed) -> {name: device tensor} (called outside any stream context; seed 0 the real problem, seed 1 the
    decoy: same shapes and dtypes, a valid problem of its own).
    call(live, ctx) -> outputs (tensors, host scalars, or dicts / tuples / dataclasses of them).  It reads the tensors
    of `live` when it runs; a buffer it updates in place is named in its outputs.
    open(live) -> ctx: handles the call needs (created on the current stream, real inputs in `live`); close(ctx).  A
    handle with state of its own (RNG counters, KMC state, history) takes that state from `live` inside call: it then
    starts every call from the same state and receives it through the delayed producer like any other input.
    fns: the entry points the CHECKED call makes, which decide whether the case may block (SYNCHRONISES); blocks=False:
    the call uses the non-blocking form of an entry point that synchronises on a condition."""
    name: str
    make: object
    call: object
    fns: tuple = ()
    open: object = None
    close: object = None
    blocks: object = None


def _fill_outputs(live, *flats):
    """the sentinel into every output tensor that is not one of the live inputs (the blocks go back to the side stream's
    pool when the caller drops them: the checked call's outputs are allocated from them)"""
    inputs_at = {t.data_ptr() for t in live.values()}
    for flat in flats:
        for v in flat.values():
            if isinstance(v, torch.Tensor) and v.numel() and v.is_contiguous() and v.data_ptr() not in inputs_at:
                v.view(-1).view(torch.uint8).fill_(SENTINEL)


def _run(case, inputs):
    """open, call, close on the current stream with copies of `inputs` -> frozen outputs"""
    live = {k: v.clone() for k, v in inputs.items()}
    ctx = case.open(live) if case.open else None
    try:
        out = freeze(_flatten(case.call(live, ctx)))
        torch.cuda.current_stream().synchronize()
    finally:
        if case.close and ctx is not None:
            case.close(ctx)
    return out


def run_on_side_stream(case, side, cycles_per_ms, synchronises):
    """-> dict(blocked=, host_ms=, delay_ms=) after asserting the bits.  `synchronises`: the case may block the host."""
    real, decoy = case.make(0), case.make(1)
    assert real.keys() == decoy.keys()
    for k in real:
        assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype and real[k].is_cuda, k
    torch.cuda.synchronize()
    # null-stream reference, and the decoy's answer: a case that cannot tell them apart proves nothing
    ref = _run(case, real)
    dref = _run(case, decoy)
    assert differing(ref, dref), "%s: the decoy gives the real outputs -- the case is blind" % case.name
    torch.cuda.synchronize()

    with recorded(), torch.cuda.stream(side):
        live = {k: v.clone() for k, v in real.items()}
        ctx = case.open(live) if case.open else None
        try:
            # warm calls at the real sizes: every grow-only buffer, pinned word and allocator block exists afterwards;
            # the second one is timed (the first pays for the allocations)
            warm = _flatten(case.call(live, ctx))
            side.synchronize()
            for k in live:
                live[k].copy_(real[k])
            side.synchronize()
            t0 = time.perf_counter()
            warm2 = _flatten(case.call(live, ctx))
            host_ms = (time.perf_counter() - t0) * 1e3
            side.synchronize()
            assert_same(freeze(warm2), ref, "%s (warm call, nothing delayed)" % case.name)
            want_ms = delay_ms_for(host_ms)
            if want_ms > MAX_DELAY_MS:
                assert synchronises, ("%s: a warm call costs the host %.1f ms, the delay rule asks for %.0f ms > %.0f ms: "
                                      "the case belongs in SYNCHRONISES with that reason" %
                                      (case.name, host_ms, want_ms, MAX_DELAY_MS))
                want_ms = MAX_DELAY_MS
            # prepare: the decoy in the live inputs AND, through one call on it, in everything the library keeps between
            # its launches (handle workspaces, thread-local scratch: a stray launch of the checked call that reads an
            # intermediate finds the decoy's there, not the warm call's); a sentinel in every output buffer that is not
            # an input; the decoy once more (the call updates some inputs in place)
            for k in live:
                live[k].copy_(decoy[k])
            warm3 = _flatten(case.call(live, ctx))
            side.synchronize()
            _fill_outputs(live, warm, warm2, warm3)
            del warm, warm2, warm3
            for k in live:
                live[k].copy_(decoy[k])
            side.synchronize()
            # the checked call: behind a sleeping producer that delivers the real inputs
            torch.cuda._sleep(int(want_ms * cycles_per_ms))
            for k in live:
                live[k].copy_(real[k])
            t0 = time.perf_counter()
            out = case.call(live, ctx)
            call_ms = (time.perf_counter() - t0) * 1e3
            busy = not side.query()
            got = _clone(_flatten(out))
            side.synchronize()
        finally:
            if case.close and ctx is not None:
                case.close(ctx)
            side.synchronize()
    info = dict(host_ms=round(host_ms, 3), delay_ms=round(want_ms, 1), call_ms=round(call_ms, 3), busy_after=busy,
                blocked=call_ms >= 0.5 * want_ms)
    REPORT["cases"][case.name] = info
    REPORT["longest_delay_ms"] = max(REPORT["longest_delay_ms"], want_ms)
    print("stream case %-44s %s" % (case.name, info))
    assert_same(freeze(got), ref, case.name)
    if synchronises:
        # (a blocking call waits for the producer: had it returned early, the table would hold a name it need not)
        assert info["blocked"], "%s is listed as synchronising but returned in %.2f ms behind a %.0f ms producer" % (
            case.name, call_ms, want_ms)
    else:
        # the producer still sleeps: the call returned without waiting for it, and was enqueued ahead of its inputs
        assert busy, "%s blocked the host: the stream had drained when the call returned (%.1f ms, delay %.0f ms)" % (
            case.name, call_ms, want_ms)
    return info
