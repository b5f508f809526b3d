"""A closed gate in front of a library call: the harness of tests/test_gpu_stream_contract.py.

include/mmf_hg.h promises that every entry enqueues on the caller's stream and nothing else.  On the idle legacy default
stream every way of breaking that promise is invisible, so a case runs the call on a busy, non-blocking side stream:

    X      <- decoy                     (default stream, then a device synchronisation; VALID data of the same shape)
    gate                                 a bounded delay enqueued on the side stream (torch.cuda._sleep, calibrated)
    X      <- truth ; produced.record    the producer sits BEHIND the gate
    (a) the gate must still be closed here, else the case FAILS with "gate too short"
    out = entry(X, ...)
    (b) entries documented as not synchronising must have returned while the gate was closed; then the host heap is churned
    side.synchronize()
    out must equal, bit for bit, the same call made beforehand on the idle default stream, and the CPU reference

Work enqueued off the stream, or a host read before the stream was synchronised, sees the decoy (or an unwritten buffer); a
host table read after its owner died sees the churned heap.  Decoys and churn are valid, finite, zero-filled data: a defect
gives a wrong answer, never a wild address.  One host thread, at most two side streams, no graph capture.

A plain helper module like tests/memh5.py, not a conftest.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

GATE_MIN_MS = 200.0          # a case's gate lasts max(GATE_MIN_MS, GATE_HOST_FACTOR x host wall time of the idle call) ...
GATE_HOST_FACTOR = 4.0       # ... the factor covers a shared, noisy host ...
GATE_MAX_MS = 3000.0         # ... and is capped here.  Never tuned to make a case pass: checks (a) and (b) guard it.
CALIBRATE_MS = 20.0          # the calibration doubles the delay until it lasts this long

RECORD: List[str] = []       # one line per case (profiles/stream_contract.txt is a copy of a run's lines)

_state = {"cycles_per_ms": None, "kind": None, "streams": None, "matmul": None}


def note(line: str) -> None:
    RECORD.append(line)
    print("[streamgate] " + line, flush=True)


def _delay(units: int) -> None:
    """The bounded delay on the current stream: `units` cycles of torch.cuda._sleep, or that many chained matmuls."""
    if _state["kind"] == "sleep":
        torch.cuda._sleep(int(units))
    else:
        a, b = _state["matmul"]
        for _ in range(int(units)):
            torch.mm(a, b, out=a)


def calibrate() -> float:
    """Units of delay per millisecond on this GPU (measured once per process with events on the default stream)."""
    if _state["cycles_per_ms"] is not None:
        return _state["cycles_per_ms"]
    if hasattr(torch.cuda, "_sleep"):
        _state["kind"], units = "sleep", 1 << 20
    else:
        _state["kind"], units = "matmul", 8
        _state["matmul"] = (torch.zeros((2048, 2048), device="cuda"), torch.zeros((2048, 2048), device="cuda"))
    torch.cuda.synchronize()
    _delay(units)                                      # the first launch loads the kernel
    torch.cuda.synchronize()
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _delay(units)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= CALIBRATE_MS or units >= (1 << 40):
            break
        units *= 2
    _state["cycles_per_ms"] = units / ms
    note(f"calibration: kind={_state['kind']} units={units} lasted {ms:.3f} ms -> {units / ms:.1f} units per ms")
    return _state["cycles_per_ms"]


def streams():
    """The two side streams of the process (non-blocking, as all of torch's): with the default stream 3 of the 4 hardware queues."""
    if _state["streams"] is None:
        _state["streams"] = (torch.cuda.Stream(), torch.cuda.Stream())
    return _state["streams"]


class Gate:
    """A delay of `ms` enqueued on `stream`, with the events that measure it."""

    def __init__(self, stream: torch.cuda.Stream, ms: float):
        self.stream, self.asked_ms = stream, float(ms)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        units = max(1, int(calibrate() * ms))
        with torch.cuda.stream(stream):
            self.e0.record(stream)
            _delay(units)
            self.e1.record(stream)

    def closed(self) -> bool:
        return not self.e1.query()

    def measured_ms(self) -> float:
        self.e1.synchronize()
        return self.e0.elapsed_time(self.e1)


def gate_ms_for(host_ms: float) -> float:
    return min(GATE_MAX_MS, max(GATE_MIN_MS, GATE_HOST_FACTOR * host_ms))


def churn() -> None:
    """Allocate, fill and drop zero-filled host buffers of 4 KiB .. 32 MiB: whatever the call freed on return is handed out
    again and overwritten with zeros (a stale offset table then decodes to in-range offsets)."""
    sizes = [4 << 10, 16 << 10, 64 << 10, 200 << 10, 1 << 20, 3 << 20, 8 << 20, 32 << 20]
    for rep in range(4):
        keep = []
        for s in sizes:
            for _ in range(4 if s <= (1 << 20) else 1):
                b = np.empty(s + 64 * rep, dtype=np.uint8)
                b.fill(0)
                keep.append(b)
            t = torch.empty(s // 8, dtype=torch.int64)       # torch's host allocator, the one that owned the wrappers' tables
            t.zero_()
            keep.append(t)
        del keep


# ---------------------------------------------------------------------------------------------------
# bit-for-bit comparison of nested results
# ---------------------------------------------------------------------------------------------------
def to_host(obj):
    """Tensors -> numpy (bf16 / f16 upcast exactly), containers kept, Python values as they are."""
    if isinstance(obj, torch.Tensor):
        t = obj.detach().cpu()
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.float()
        return t.numpy().copy()
    if isinstance(obj, dict):
        return {k: to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_host(v) for v in obj]
    return obj


def _bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def diff(got, want, where: str = "out", atol: float = 0.0) -> List[str]:
    """Mismatches between two nested host results; bit for bit (NaN equals the same NaN), or to `atol` for float arrays (where
    any NaN equals any NaN: 0 / 0 on the device carries the sign bit, numpy's nan does not)."""
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        g, w = np.asarray(got), np.asarray(want)
        if g.shape != w.shape:
            return [f"{where}: shape {g.shape} != {w.shape}"]
        if g.dtype != w.dtype:
            return [f"{where}: dtype {g.dtype} != {w.dtype}"]
        if atol and g.dtype.kind == "f":
            with np.errstate(invalid="ignore"):
                bad = ~((np.abs(g.astype(np.float64) - w.astype(np.float64)) <= atol) | (_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = _bits(g) != _bits(w)
        n = int(np.count_nonzero(bad))
        return [f"{where}: {n} of {g.size} values differ"] if n else []
    if isinstance(want, dict):
        if not isinstance(got, dict) or sorted(got) != sorted(want):
            return [f"{where}: keys differ"]
        return [m for k in want for m in diff(got[k], want[k], f"{where}[{k!r}]", atol)]
    if isinstance(want, (list, tuple)):
        if not isinstance(got, (list, tuple)) or len(got) != len(want):
            return [f"{where}: length differs"]
        return [m for i, (g, w) in enumerate(zip(got, want)) for m in diff(g, w, f"{where}[{i}]", atol)]
    if isinstance(want, float) and isinstance(got, float):
        same = (got == want) or (got != got and want != want) or (atol and abs(got - want) <= atol)
        return [] if same else [f"{where}: {got!r} != {want!r}"]
    return [] if got == want else [f"{where}: {got!r} != {want!r}"]


def _against(got, want, atol: float) -> List[str]:
    """`want` is the expected result, or a check: callable(got) -> list of mismatches (a reference that pins only part of it)."""
    return list(want(got)) if callable(want) else diff(got, want, atol=atol)


# ---------------------------------------------------------------------------------------------------
@dataclass
class Gated:
    name: str
    mismatches: List[str] = field(default_factory=list)
    gate_ms: float = 0.0           # measured with events
    host_ms: float = 0.0           # wall time of the same call on the idle default stream
    returned_closed: Optional[bool] = None     # the entry came back while the gate was closed (None: not asked)
    out: object = None             # the gated call's result on the host


def run_gated(entry: Callable, make_inputs: Callable[[str], Sequence[torch.Tensor]], reference: Optional[Callable], *,
              name: str, nonsync: bool = False, atol: float = 0.0, calls: int = 1, finish: Optional[Callable] = None,
              report: bool = False, side: Optional[torch.cuda.Stream] = None) -> Gated:
    """One case of the stream contract.

    entry(*device_tensors) -> a tensor / nested container of tensors and Python values: the call under test, made with the
        current torch stream.  It is made on the idle default stream first (the bits to reproduce, and the host wall time
        that sizes the gate), then on the busy side stream behind the gate, `calls` times in a row (a second call whose
        memsets ran off the stream finds the workspace the first one dirtied).
    make_inputs("truth" | "decoy") -> the CPU tensors that become the entry's device arguments.  The decoy is valid data of
        the same shapes and dtypes.
    reference(*truth as numpy) -> the expected result as a nested host structure (compared bit for bit, float arrays to
        `atol` when given), or a check callable(result on the host) -> list of mismatches, or None (the idle call's bits only).
    nonsync: the entry is documented as not synchronising with the host: check (b) and the heap churn apply.
    finish(out) -> out: what a caller does AFTER the stream has been synchronised (say, reading a count); applied to the idle
        and the gated result alike before they are compared.
    report: return the Gated record with its mismatches instead of raising (the harness's self-test).
    """
    side = side or streams()[0]
    truth = [t.contiguous() for t in make_inputs("truth")]
    decoy = [t.contiguous() for t in make_inputs("decoy")]
    assert len(truth) == len(decoy) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(truth, decoy)), \
        f"{name}: the decoy must have the shapes and dtypes of the truth"
    pinned = [t.pin_memory() for t in truth]           # a non_blocking copy out of pageable memory would wait for the gate
    res = Gated(name)

    # ---- the idle default stream: the bits to reproduce, the host wall time, the reference ----------------------
    idle_in = [t.cuda() for t in truth]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idle_dev = entry(*idle_in)
    torch.cuda.synchronize()
    res.host_ms = (time.perf_counter() - t0) * 1e3
    if finish is not None:
        idle_dev = finish(idle_dev)
    idle = to_host(idle_dev)
    keep = [idle_dev, idle_in]                          # alive until the case ends: a freed block with the right answer in
    if reference is not None:                           # it must not be handed to the call under test
        want = reference(*[t.float().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.numpy() for t in truth])
        res.mismatches += [f"idle default stream vs reference: {m}" for m in _against(idle, want, atol)]

    # ---- the busy side stream ---------------------------------------------------------------------------------
    X = [t.cuda() for t in decoy]
    torch.cuda.synchronize()
    if nonsync:
        # A cached (device, stream) workspace that has to grow synchronises the stream by contract (mmf_host.h), whatever the
        # entry: one ungated call on the decoy gives the side stream's workspace its size, so that check (b) sees the entry
        # itself and does not depend on which cases ran before this one.
        with torch.cuda.stream(side):
            warm = entry(*X)
            side.synchronize()
        keep.append(warm)
    ms = gate_ms_for(res.host_ms)
    gate = Gate(side, ms)
    produced = torch.cuda.Event()
    outs = []
    with torch.cuda.stream(side):
        for x, t in zip(X, pinned):
            x.copy_(t, non_blocking=True)
        produced.record(side)
        open_at_start = not produced.query()            # (a)
        if open_at_start:
            for _ in range(calls):
                outs.append(entry(*X))
            if nonsync:
                res.returned_closed = not produced.query()      # (b)
                churn()
        side.synchronize()
        if finish is not None:
            outs = [finish(o) for o in outs]
    res.gate_ms = gate.measured_ms()
    note(f"case {name}: gate {res.gate_ms:.1f} ms (asked {ms:.1f}), host {res.host_ms:.2f} ms, "
         f"{'returned while the gate was closed' if res.returned_closed else 'synchronised' if res.returned_closed is None else 'DID NOT return while the gate was closed'}")
    if not open_at_start:
        raise AssertionError(f"{name}: gate too short: the producer had run before the call started "
                             f"(gate measured {res.gate_ms:.1f} ms, host {res.host_ms:.2f} ms)")
    for c, o in enumerate(outs):
        got = to_host(o)
        res.out = got
        res.mismatches += [f"gated call {c} vs idle default stream: {m}" for m in diff(got, idle)]
        if reference is not None:
            res.mismatches += [f"gated call {c} vs reference: {m}" for m in _against(got, want, atol)]
    if nonsync and not res.returned_closed:
        res.mismatches.append(f"documented as not synchronising, but returned only after the gate opened "
                              f"(gate {res.gate_ms:.1f} ms, host {res.host_ms:.2f} ms)")
    del keep
    if res.mismatches and not report:
        raise AssertionError(f"{name}: " + "; ".join(res.mismatches[:8]))
    return res
