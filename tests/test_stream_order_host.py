"""The capture / replay driver (tests/stream_driver.py) has teeth: over a fake backend on CPU tensors -- capture records the closure,
replay calls it -- it passes a correct entry point and fails every wrong one at the step that is meant to find it.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_driver as D  # noqa: E402

N, PITCH = 37, 48            # a ragged tail: columns 37..47 of each row are pad and stay unwritten


class FakeBackend:
    device = "cpu"

    def __init__(self):
        self.capturing = False

    def capture(self, fn):
        """fn is called once in capture mode; what it returns then is the recorded work (a real capture records launches, not Python)."""
        self.capturing = True
        try:
            return fn()
        finally:
            self.capturing = False

    def replay(self, handle):
        handle()

    def sync(self):
        pass

    def before_capture(self):
        return None

    def after_capture(self, token):
        pass

    def status(self):
        return 0


def f(x):
    return (x.to(torch.int32) * 3 + 1).to(torch.uint8) & 0x7F        # never 0xEE


def entry(kind, backend):
    """build(arena) of a fake entry point out[r, :N] = f(in[r, :N]) plus an in-place counter row; `kind` names its defect."""
    def build(arena):
        src = arena.input((2, PITCH))
        out = arena.output((2, PITCH))
        acc = arena.state((PITCH,))
        sets = {"A": torch.arange(2 * PITCH, dtype=torch.uint8).reshape(2, PITCH), "B": (torch.arange(2 * PITCH, dtype=torch.uint8).reshape(2, PITCH) * 7 + 5)}
        start = {"A": torch.full((PITCH,), 3, dtype=torch.uint8), "B": torch.full((PITCH,), 9, dtype=torch.uint8)}
        host = {"calls": 0}

        def work(x, cols=N):
            host["calls"] += 1
            prior = out[:, :cols].clone()
            res = f(x[:, :cols])
            if kind == "reads_output":
                res = res | (prior & 1)
            if kind == "reads_output_zero":
                res = res + (prior == 0).to(torch.uint8)
            if kind == "host_counter" and host["calls"] >= 5:
                res = res + 1
            out[:, :cols] = res
            acc[:cols] += 1

        def call():
            if backend.capturing:
                if kind == "works_at_capture":
                    work(src)
                if kind == "only_at_call_time":
                    return lambda: None
                if kind == "snapshots_input":
                    frozen = src.clone()
                    return_work = lambda: work(frozen)      # noqa: E731
                    return return_work
                if kind == "skips_tail_on_replay":
                    return lambda: work(src, N - 1)
                return lambda: work(src)
            work(src)
            return None

        def fill(which):
            src.copy_(sets[which])
            acc.copy_(start[which])

        def check(which):
            assert torch.equal(out[:, :N], f(sets[which][:, :N])), "out"
            assert torch.equal(acc[:N], start[which][:N] + 1) and torch.equal(acc[N:], start[which][N:]), "acc"

        return D.Built(call, fill, check)
    return build


def drive(kind):
    backend = FakeBackend()
    D.run(backend, entry(kind, backend))


def test_a_correct_entry_point_passes():
    drive("correct")


@pytest.mark.parametrize("kind,step", [
    ("works_at_capture", 4),          # does its work at capture time as well
    ("only_at_call_time", 5),         # nothing is recorded
    ("snapshots_input", 6),           # input contents frozen at capture time
    ("reads_output", 7),              # out = f(in) | (out_before & 1): bit 0 of the fills 0xEE and 0x00 is clear, 0xFF (step 7) sets it
    ("reads_output_zero", 6),         # reads its output's prior contents in a way the zero fill of step 6 shows
    ("skips_tail_on_replay", 5),      # one ragged-tail column unwritten, only when replayed
    ("host_counter", 7),              # host-side state changes the result of a later replay
])
def test_each_wrong_entry_point_fails_at_its_step(kind, step):
    with pytest.raises(D.StepFailed) as e:
        drive(kind)
    assert e.value.step == step, str(e.value)


def test_float_payload_rows_tell_written_0xEE_from_poison():
    """A row whose written bytes can be 0xEE: the 0xEE and 0xFF fills together identify the footprint, and a write outside it fails."""
    def build(extra):
        def b(arena):
            out = arena.output((PITCH,))
            src = arena.input((PITCH,))
            sets = {"A": torch.full((PITCH,), 0xEE, dtype=torch.uint8), "B": torch.full((PITCH,), 0x21, dtype=torch.uint8)}
            rec = {"replays": 0}

            def call():
                def work():
                    out[:N] = src[:N]
                    if extra and rec["replays"] == 3:               # the replay of step 6 alone
                        out[N] = 0x55
                    rec["replays"] += 1
                return work
            eager = lambda: call()()        # noqa: E731
            built = D.Built(None, lambda which: src.copy_(sets[which]), lambda which: None, float_payload=True)
            built.call = lambda: call() if backend.capturing else (eager(), None)[1]
            return built
        return b
    backend = FakeBackend()
    D.run(backend, build(False))
    backend = FakeBackend()
    with pytest.raises(D.StepFailed) as e:
        D.run(backend, build(True))
    assert e.value.step == 6


def test_a_table_outside_the_arena_is_checked_after_every_replay():
    """after_replay: a side table the byte comparisons leave out (slot order is free) is compared as a set after every replay; an entry
    point that fills it when called but not when replayed fails at step 5."""
    def build(forget):
        def b(arena):
            out, src = arena.output((PITCH,)), arena.input((PITCH,))
            table = torch.zeros(8, dtype=torch.uint8)                  # plain: not in the arena
            sets = {"A": torch.full((PITCH,), 4, dtype=torch.uint8), "B": torch.full((PITCH,), 9, dtype=torch.uint8)}

            def work(with_table):
                out[:N] = src[:N] + 1
                if with_table:
                    table[torch.randperm(8)[:2]] = src[0]              # two entries, wherever they land

            def call():
                if backend.capturing:
                    return lambda: work(not forget)
                work(True)

            def fill(which):
                src.copy_(sets[which])
                table.zero_()

            def table_is(which):
                assert sorted(table.tolist()) == [0] * 6 + [int(sets[which][0])] * 2, "table"
            return D.Built(call, fill, lambda which: (table_is(which), None)[1], after_replay=table_is)
        return b
    backend = FakeBackend()
    D.run(backend, build(False))
    backend = FakeBackend()
    with pytest.raises(D.StepFailed) as e:
        D.run(backend, build(True))
    assert e.value.step == 5


# ------------------------------------------------------------------------------------------------- the case table is complete
def test_every_launching_export_has_a_capture_case():
    """Every export the bindings' signature tables declare is a row of tests/stream_cases.py or is excluded there with a reason: a
    new export without a capture case fails here."""
    import stream_cases as C
    rows = {r.export for r in C.ROWS}
    tables = C.signature_tables()
    assert set(tables) == {"_lib", "_episode_lib", "_cubie_lib", "_search_lib", "_astar_lib", "_sym_lib", "_pattern_lib", "_net_lib"}
    exports = set()
    for name, table in tables.items():
        for fn in table:
            assert (fn in rows) != (fn in C.EXCLUDED), f"{name}.{fn}: " + ("both a row and excluded" if fn in rows else "no capture case and no exclusion")
            exports.add(fn)
    assert rows <= exports and set(C.EXCLUDED) <= exports, sorted((rows | set(C.EXCLUDED)) - exports)
    assert all(isinstance(why, str) and why.strip() and "\n" not in why for why in C.EXCLUDED.values())
    # what the table must hold beyond one row per name
    variants = {r.export: set() for r in C.ROWS}
    sizes = {r.export: set() for r in C.ROWS}
    for r in C.ROWS:
        variants[r.export] |= set(r.variants)
        sizes[r.export] |= set(r.cube_sizes)
    assert variants["rc_scramble"] >= {"replay", "drawn"} and variants["rcs_sym_apply"] == {"one", "per_cube"}
    assert variants["rc_legacy_scramble_actions_ex"] == {0, 1, 2 + 16 * 7}
    assert len(variants["rc_net_first_layer"]) == 8 and variants["rc_search_select"] >= {"40x5", "3x300"}
    assert variants["rcp_build_level"] == set(range(15)) and sizes["rcp_build_level"] == {2, 3}
    three_only = {"rc_onehot_from_family", "rc_onehot_from_family_depths"}           # the family -> dense writer has no 2x2x2 form
    assert all(sizes[e] == ({3} if e in three_only else {2, 3}) for e in sizes), sizes
    ids = [c[0] for c in C.cases()]
    assert len(ids) == len(set(ids))
