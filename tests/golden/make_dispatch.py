#!/usr/bin/env python3
"""Fixture for tests/test_host_logic.py::test_dispatch_fixture_replays: what rc_describe_dispatch answers, query by query.

rc_describe_dispatch formats the plan the launchers run (csrc/rubikhip.hip plan_*), so this file pins every launch decision of the
library -- kernel form, template selectors, grid, block, parts, segments -- without a GPU.  One line per query:

    op cube_size n depth outputs fmt variant <TAB> the string, or !<return code> where the call is refused

Run it on the build whose dispatch is to be pinned (a change of a threshold regenerates the file, and the diff of dispatch.txt
then IS the review of the policy change); RUBIKHIP_LIB + RC_ALLOW_STALE=1 select another build's library:

    python tests/golden/make_dispatch.py                       writes tests/golden/dispatch.txt (the committed subset, < 200 KB)
    python tests/golden/make_dispatch.py --sweep OUT.txt       the exhaustive grid (about 1.8 M lines): run it with two builds and diff

The sweep crosses every op, both cube sizes, every n of N, depth 1 / 5 / 30, every fmt, every combination of the RC_OUT_* bits the
op reads and variant 0 or one accepted value of one RC_VARIANT_* field of the op's group, then adds the field combinations the GPU
tests launch and some refused values.  The fixture keeps, at variant 0, every n x format x the output sets that reach a different
plan (a bit the plan of that op and format never reads is left clear; 2x2x2 has no workspace route and no family writer), and every
variant field value at two sizes (4096 and 2^20; ADI 3000 x 7 and 100000 x 30)."""
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from rubiks_cube_solver_amd import _lib as L  # noqa: E402

N = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 1 << 14, (1 << 15) - 1, 1 << 15, (1 << 16) - 1, 1 << 16, (1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18,
     (1 << 19) - 1, 1 << 19, 1 << 20, (1 << 20) + 3, 1 << 22, 1 << 24, 43008, 100000, 20000]
FMTS = (L.FMT_NONE, L.FMT_CODE, L.FMT_U8, L.FMT_F16, L.FMT_F32, L.FMT_BF16)
DENSE = FMTS[2:]
S, C, F, R, I, D, W, FAM = L.OUT_STATES, L.OUT_CODE, L.OUT_FLAGS, L.OUT_REWARD, L.OUT_INPLACE, L.OUT_DONE, L.OUT_WORKSPACE, L.OUT_FAMILY
OPS = (L.OP_STEP, L.OP_EXPAND, L.OP_ADI, L.OP_CODE_TO_DENSE, L.OP_FAMILY_TO_DENSE)
READS = {L.OP_STEP: (S, C, R, I, D, W), L.OP_EXPAND: (S, C), L.OP_ADI: (S, C, F, FAM), L.OP_CODE_TO_DENSE: (), L.OP_FAMILY_TO_DENSE: ()}

# unknown op, cube size, n = 0, depth = 0
REFUSED = [(0, 3, 10, 1, 0, 0, 0), (6, 3, 10, 1, 0, 0, 0), (1, 4, 10, 1, 0, 0, 0), (1, 3, 0, 1, 0, 0, 0), (3, 3, 10, 0, 0, 0, 0), (5, 3, 10, 0, 0, 4, 0)]


def subsets(bits):
    return [sum(c) for k in range(len(bits) + 1) for c in itertools.combinations(bits, k)]


def variants(op, cube):
    """Every accepted value of every RC_VARIANT_* field of op's group, one field at a time (fields of a dense form with that form)."""
    A = 6 if cube == 2 else 12
    if op == L.OP_STEP:
        return [1, 2] + [10 * p for p in range(1, 5)] + [100000, 200000]
    if op == L.OP_EXPAND:
        return [1, 2] + [100 * h for h in range(1, 9)] + [1000 * p for p in range(1, A + 1)]
    if op == L.OP_ADI:
        return [1, 2] + [1000 * p for p in range(1, A + 1)] + [1000000 * s for s in range(1, 17)]
    if op == L.OP_CODE_TO_DENSE:
        front = [1, 2, 4, 20, 30, 40]
        return [100000, 200000, 300000, 400000] + front + [400000 + f for f in front] + [300000 + 10 * k for k in range(1, 10)] + \
               [300000 + 1000 * g for g in range(1, 100)]
    return []


def tested_and_refused(op, cube):
    """Field combinations the GPU tests launch (tests/test_gpu_dispatch.py), and values every entry point must refuse."""
    A = 6 if cube == 2 else 12
    bad = [-1, 3, 100000000, 2000000000]
    if op == L.OP_STEP:
        return [v + 10 * p + 100000 * t for v in range(3) for p in range(5) for t in range(3)] + bad + [50, 100, 1000, 300000, 1000000]
    if op == L.OP_EXPAND:
        return [1000 * p + v for p in range(A + 1) for v in range(3)] + [100 * h + v for h in range(1, 9) for v in (1, 2)] + bad + [10, 900, 1000 * (A + 1), 100000]
    if op == L.OP_ADI:
        return [1000000 * s + 1000 * p + v for s in range(17) for p in (0, 1, 2, 3, 4, 6, 12)[:5 if cube == 2 else 7] for v in range(3)] + \
               bad + [10, 100, 1000 * (A + 1), 100000, 17000000, 40000001]
    if op == L.OP_CODE_TO_DENSE:
        return [f + u + 10 * t for f in (0, 400000) for u in (0, 1, 2, 4) for t in (0, 2, 3, 4)] + [300000 + 1000 * g + 10 * k for g in (1, 7, 8) for k in (1, 3)] + \
               bad + [10, 100, 1000, 100001, 201000, 300001, 500000, 1000000]
    return [1, 10, 1000, 100000]


def sweep():
    for op, cube in itertools.product(OPS, (2, 3)):
        outs = subsets(READS[op])
        for n, depth, fmt, o in itertools.product(N, (1, 5, 30), FMTS, outs):
            for v in [0] + variants(op, cube):
                yield op, cube, n, depth, o, fmt, v
        for n, fmt, o, v in itertools.product((2500, 3000, 4096, 9000, 100000, 1 << 20), FMTS, outs, tested_and_refused(op, cube)):
            yield op, cube, n, 7, o, fmt, v
    yield from REFUSED


def fixture():
    adi_outs = (S | F, C | F, FAM | F, S | C | F, C)
    for n in N:
        for cube in (3, 2):
            for o in (S | D, S | D | R, D, S | I | D, S | C | D | R)[:5 if cube == 3 else 2]:
                yield L.OP_STEP, cube, n, 0, o, L.FMT_NONE, 0
            for o in (0, S | D | R, S | I | D | R)[:3 if cube == 3 else 1]:
                yield L.OP_STEP, cube, n, 0, o, L.FMT_CODE, 0
            for fmt in DENSE:
                for o in (S, 0, S | W | D | R, W)[:4 if cube == 3 else 1]:
                    yield L.OP_STEP, cube, n, 0, o, fmt, 0
                yield L.OP_CODE_TO_DENSE, cube, n, 0, 0, fmt, 0
            for o in (S, S | C, C)[:3 if cube == 3 else 2]:
                yield L.OP_EXPAND, cube, n, 0, o, L.FMT_NONE, 0
            for o in adi_outs[:5 if cube == 3 else 2]:
                yield L.OP_ADI, cube, n, 30, o, L.FMT_NONE, 0
        for fmt in DENSE:
            yield L.OP_FAMILY_TO_DENSE, 3, n, 30 if n in (257, 43008) else 1, 0, fmt, 0
    for n, o in itertools.product((257, 3000, 20000, 100000, 1 << 20), adi_outs):
        for depth in (1, 5):
            yield L.OP_ADI, 3, n, depth, o, L.FMT_NONE, 0
    for n in (4096, 1 << 20):
        for v in variants(L.OP_STEP, 3) + tested_and_refused(L.OP_STEP, 3)[-9:]:
            for o, fmt in ((S | D, L.FMT_NONE), (S | D | R, L.FMT_CODE), (S, L.FMT_BF16), (S | W, L.FMT_F32)):
                yield L.OP_STEP, 3, n, 0, o, fmt, v
        for cube in (3, 2):
            for v in variants(L.OP_EXPAND, cube) + tested_and_refused(L.OP_EXPAND, cube)[-8:]:
                for o in (S, S | C):
                    yield L.OP_EXPAND, cube, n, 0, o, L.FMT_NONE, v
        for v in variants(L.OP_CODE_TO_DENSE, 3) + tested_and_refused(L.OP_CODE_TO_DENSE, 3):
            if v < 301000 or v >= 400000 or n > 4096:                  # the wide form's group counts: at 2^20 cubes only
                yield L.OP_CODE_TO_DENSE, 3, n, 0, 0, L.FMT_BF16, v
        for v in variants(L.OP_CODE_TO_DENSE, 3)[:16]:
            yield L.OP_CODE_TO_DENSE, 3, n, 0, 0, L.FMT_F32, v
        for v in variants(L.OP_CODE_TO_DENSE, 2)[:10]:
            yield L.OP_CODE_TO_DENSE, 2, n, 0, 0, L.FMT_U8, v
        yield L.OP_FAMILY_TO_DENSE, 3, n, 2, 0, L.FMT_F32, 1
    for n, depth in ((3000, 7), (100000, 30)):
        for cube in (3, 2):
            for v in variants(L.OP_ADI, cube) + tested_and_refused(L.OP_ADI, cube)[-10:]:
                for o in (S | F, C | F, FAM | F)[:3 if cube == 3 else 2]:
                    yield L.OP_ADI, cube, n, depth, o, L.FMT_NONE, v
    yield from REFUSED


def answer(q):
    import ctypes
    buf = ctypes.create_string_buffer(160)
    rc = L.lib().rc_describe_dispatch(*q, buf, len(buf))
    return buf.value.decode() if rc == 0 else f"!{rc}"


def write(path, queries):
    seen = set()
    with open(path, "w") as f:
        for q in queries:
            if q not in seen:
                seen.add(q)
                f.write(" ".join(map(str, q)) + "\t" + answer(q) + "\n")
    print(f"{path}: {len(seen)} queries, {os.path.getsize(path)} bytes from library {L.build_id()}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--sweep"]:
        write(sys.argv[2], sweep())
    else:
        write(os.path.join(HERE, "dispatch.txt"), fixture())
