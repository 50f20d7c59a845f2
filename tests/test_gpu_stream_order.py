"""include/rubikhip.h: "Calls are stream-ordered, never synchronise (except rc_read_status, rc_facade_step(wait=1) and rc_get_tables),
are re-entrant, and keep no mutable state besides the per-device status word" -- held for EVERY launching entry point of librubikhip,
librubiksearch and librubiknet, one call at a time, under hipGraph capture and replay.  GPU only.

Per row of tests/stream_cases.py and cube size, tests/stream_driver.py: eager runs on two input sets against the row's reference;
ONE call captured on a side stream (nothing may be written, no workspace cached); replay on set A = the eager bytes, guards and pad
columns included; replay over zeroed buffers on set B; replay over 0xFF on set A again; a clean status word.  A launch that misses the
passed stream breaks the capture or is missing from the replay, host work at call time is missing from the replay, a hidden
synchronisation or allocation is an error during capture: no timing is involved.  tests/test_stream_order_host.py proves the driver on
the CPU and holds the table complete."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as C  # noqa: E402
import stream_driver as D  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = C.cases()


class GraphBackend:
    """capture: torch.cuda.graph on a side stream in the default (global) error mode, single-stream and linear."""
    device = "cuda"

    def __init__(self, ops, L):
        self.ops, self.L = ops, L

    def sync(self):
        torch.cuda.synchronize()

    def before_capture(self):
        return dict(self.ops._workspaces)

    def after_capture(self, cached):
        now = self.ops._workspaces
        D.need(set(now) == set(cached) and all(now[k] is v for k, v in cached.items()), 4, "the capture changed ops._workspaces")

    def capture(self, call):
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                call()
        torch.cuda.current_stream().wait_stream(side)
        return g

    def replay(self, g):
        g.replay()

    def status(self):
        return self.L.read_status()


@pytest.fixture(scope="module")
def ctx(oracle):
    c = C.Ctx(oracle, "cuda")
    C.pattern_dist(2), C.pattern_dist(3)            # the reference distance tables, once (the 2x2x2's takes the CPU half a minute)
    return c


@pytest.mark.parametrize("row,cs,variant", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_one_call_under_capture_and_replay(ctx, row, cs, variant):
    try:
        with torch.no_grad():
            D.run(GraphBackend(ctx.ops, ctx.L), lambda arena: row.build(ctx, cs, variant, arena))
    except Exception as e:  # noqa: BLE001
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")) and "capture" not in str(e).lower():
            pytest.exit(f"a GPU fault in this case: nothing more is started on the device -- {e}", returncode=3)
        raise
