"""The capture / replay driver of tests/test_gpu_stream_order.py, written against a tiny backend so that tests/test_stream_order_host.py
can prove on the CPU that it has teeth.

include/rubikhip.h: "Calls are stream-ordered, never synchronise (...), are re-entrant, and keep no mutable state besides the per-device
status word."  run() checks that sentence for ONE call of one entry point: the call is run eagerly on two sets of inputs (A, B) against
the row's reference, captured once, and replayed three times over re-poisoned buffers and refilled inputs.

A backend has  device,  capture(callable) -> handle,  replay(handle),  sync(),  and the two hooks  before_capture() -> token,
after_capture(token)  (the GPU backend checks ops._workspaces there).  A case (tests/stream_cases.py) is built with an Arena, which
carves every output and state buffer out of a larger allocation with a 64-byte guard on each side:

    arena.output(shape, dtype)   write-only buffer
    arena.state(shape, dtype)    buffer the call updates in place; fill(which) resets it
    arena.input(shape, dtype)    plain tensor whose contents fill(which) rewrites (never reallocated)

build() returns a Built: call(), fill(which), check(which) (asserts outputs == reference(which) over what the reference defines),
optionally after_replay(which) (a set comparison of a table the byte comparisons must leave out, repeated after every replay), and
float_payload -- True where written bytes can legitimately be 0xEE.  Such rows use the fills 0xEE (step 5) and 0xFF (step 7) TOGETHER to
tell written bytes from poison: a byte is unwritten when it reads 0xEE after the first and 0xFF after the second; the footprint check
of step 6 is then made with that mask, after step 7.  Every other row uses the literal rule of step 6.
"""
import numpy as np
import torch

GUARD = 64
POISON = 0xEE


class StepFailed(AssertionError):
    def __init__(self, step, what):
        super().__init__(f"step {step}: {what}")
        self.step = step


def need(cond, step, what):
    if not cond:
        raise StepFailed(step, what)


class Arena:
    def __init__(self, device):
        self.device = device
        self.raw = []            # whole allocations of outputs and state, guards included
        self.views = []          # (kind, view)

    def _carve(self, kind, shape, dtype):
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((GUARD + size + GUARD,), POISON, dtype=torch.uint8, device=self.device)
        view = raw[GUARD:GUARD + size].view(dtype).reshape(shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 0
        self.raw.append(raw)
        self.views.append((kind, view))
        return view

    def output(self, shape, dtype=torch.uint8):
        return self._carve("output", shape, dtype)

    def state(self, shape, dtype=torch.uint8):
        return self._carve("state", shape, dtype)

    def input(self, shape, dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def poison(self, value):
        for raw in self.raw:
            raw.fill_(value)

    def snapshot(self):
        return torch.cat([raw.clone() for raw in self.raw]) if self.raw else torch.zeros(0, dtype=torch.uint8, device=self.device)

    def guards_and_outputs_are(self, value):
        for raw, (kind, _) in zip(self.raw, self.views):
            part = raw if kind == "output" else torch.cat([raw[:GUARD], raw[-GUARD:]])
            if not bool((part == value).all()):
                return False
        return True

    def state_bytes(self):
        return [raw[GUARD:-GUARD].clone() for raw, (kind, _) in zip(self.raw, self.views) if kind == "state"]


class Built:
    def __init__(self, call, fill, check, float_payload=False, after_replay=None):
        """after_replay(which): an order-independent check of what lies outside the arena (a hash table whose slot placement depends on
        the order of the lanes), made after every replay as well; None where the byte comparisons see everything."""
        self.call, self.fill, self.check, self.float_payload, self.after_replay = call, fill, check, float_payload, after_replay


def run(backend, build):
    """build(arena) -> Built.  Raises StepFailed(step, ...) with the number of the step (2..8) that found the defect."""
    arena = Arena(backend.device)
    case = build(arena)
    assert any(kind == "output" for kind, _ in arena.views) or any(kind == "state" for kind, _ in arena.views), "a case without results"

    def replayed(step, which):
        if case.after_replay is not None:
            try:
                case.after_replay(which)
            except AssertionError as e:
                raise StepFailed(step, f"after the replay on set {which}: {e}") from e

    eager = {}
    for step, which in ((2, "A"), (3, "B")):
        arena.poison(POISON)
        case.fill(which)
        case.call()
        backend.sync()
        try:
            case.check(which)
        except StepFailed:
            raise
        except AssertionError as e:
            raise StepFailed(step, f"eager run on set {which} differs from the reference: {e}") from e
        eager[which] = arena.snapshot()
    # 4. one captured call: nothing may run at capture time
    arena.poison(POISON)
    case.fill("A")
    start = arena.state_bytes()
    backend.sync()
    token = backend.before_capture()
    try:
        handle = backend.capture(case.call)
    except StepFailed:
        raise
    except Exception as e:  # noqa: BLE001 -- a capture that raises is the defect this step looks for
        raise StepFailed(4, f"the capture raised: {type(e).__name__}: {e}") from e
    backend.sync()
    need(arena.guards_and_outputs_are(POISON), 4, "an output or guard byte was written while the call was being captured")
    need(all(torch.equal(a, b) for a, b in zip(start, arena.state_bytes())), 4, "a state buffer changed while the call was being captured")
    backend.after_capture(token)
    # 5. replay on set A
    backend.replay(handle)
    backend.sync()
    snap5 = arena.snapshot()
    replayed(5, "A")
    need(torch.equal(snap5, eager["A"]), 5, f"first replay differs from the eager run in {int((snap5 != eager['A']).sum())} bytes")
    # 6. zero poison, set B
    arena.poison(0x00)
    case.fill("B")
    backend.replay(handle)
    backend.sync()
    snap6 = arena.snapshot()
    replayed(6, "B")
    written_b = eager["B"] != POISON
    need(torch.equal(snap6[written_b], eager["B"][written_b]), 6,
         f"replay on set B differs from the eager run in {int((snap6[written_b] != eager['B'][written_b]).sum())} written bytes")
    if not case.float_payload:
        unwritten_a = eager["A"] == POISON
        need(bool((snap6[unwritten_a] == 0).all()), 6, f"{int((snap6[unwritten_a] != 0).sum())} bytes outside the eager footprint were written")
    # 7. 0xFF poison, set A again
    arena.poison(0xFF)
    case.fill("A")
    backend.replay(handle)
    backend.sync()
    snap7 = arena.snapshot()
    replayed(7, "A")
    maybe = eager["A"] == POISON
    need(torch.equal(snap7[~maybe], eager["A"][~maybe]), 7,
         f"third replay differs from the eager run in {int((snap7[~maybe] != eager['A'][~maybe]).sum())} written bytes")
    if case.float_payload:
        need(bool(((snap7[maybe] == 0xFF) | (snap7[maybe] == POISON)).all()), 7, "third replay: a byte is neither poison nor the eager run's value")
        unwritten_a = maybe & (snap7 == 0xFF)
        need(bool((snap6[unwritten_a] == 0).all()), 6, f"{int((snap6[unwritten_a] != 0).sum())} bytes outside the eager footprint were written")
    else:
        need(bool((snap7[maybe] == 0xFF).all()), 7, f"third replay wrote {int((snap7[maybe] != 0xFF).sum())} bytes outside the eager footprint")
    # 8. the status word
    need(backend.status() == 0, 8, "the status word is set")
