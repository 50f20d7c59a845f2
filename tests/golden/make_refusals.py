#!/usr/bin/env python3
"""Fixture for tests/test_host_logic.py::test_refusal_fixture_replays: what the search, A*, symmetry and net entry points answer to
arguments they must refuse, call by call -- return code and the WHOLE error text.  No GPU is needed: every call is stopped by the host
checks in front of the first HIP call.  (librubikhip's plan refusals are pinned by dispatch.txt.)  One line per call:

    function arg arg ... <TAB> return code <TAB> the library's last-error text after the call

An argument is a decimal integer, a float written f:<value>, or a pointer: null, ptr / ptr2 (two distinct 16-byte aligned host
buffers) or odd (ptr + 4).  No pointer is ever dereferenced, and every call is built so that it cannot launch even if the check it
is about wrongly accepted it: a NULL buffer, an in == out pair, a table size of 0 or n == 0 stops it further down.  Where an accepted
boundary value is recorded (the largest pitch below rows * pitch = 2^32), the recorded answer IS that later refusal, or 0 at n == 0.
Cases that cannot be arranged that way (root_pitch of rc_search_init / rca_init, alignment where a launch follows) stay with the GPU tests.

Run it on the build whose refusals are to be pinned; RUBIKSEARCH_LIB / RUBIKNET_LIB + RC_ALLOW_STALE=1 select another build's libraries:

    python tests/golden/make_refusals.py                       writes tests/golden/refusals.txt"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

_BUF = ctypes.create_string_buffer(96)
_PTR = (ctypes.addressof(_BUF) + 15) & ~15
POINTERS = {"null": None, "ptr": _PTR, "ptr2": _PTR + 32, "odd": _PTR + 4}


def entry_points():
    """{function name: (CDLL, argtypes, the library's last-error function)} of the libraries the fixture covers."""
    from rubiks_cube_solver_amd import _astar_lib, _native, _net_lib, _search_lib, _sym_lib
    out = {}
    for lib, err, tables in ((_search_lib.search_lib(), "rc_search_last_error", (_search_lib.SIGNATURES, _astar_lib.ASTAR_SIGNATURES, _sym_lib.SYM_SIGNATURES)),
                             (_net_lib.net_lib(), "rc_net_last_error", (_net_lib.SIGNATURES,))):
        _astar_lib.astar_lib(), _sym_lib.sym_lib()                     # the rca_* / rcs_* signatures, applied to the same binary
        for table in tables:
            for fn, sig in table.items():
                out[fn] = (lib, _native.signature(sig)[0], getattr(lib, err))
    return out


def call(entries, query):
    """(return code, error text) of one fixture query 'function arg arg ...'; the text of a call that returns 0 is empty (the library
    keeps its last refusal's)."""
    fn, *tokens = query.split(" ")
    lib, argtypes, last_error = entries[fn]
    assert len(tokens) == len(argtypes), query
    args = [POINTERS[t] if ty is ctypes.c_void_p else float(t[2:]) if t.startswith("f:") else int(t) for t, ty in zip(tokens, argtypes)]
    rc = getattr(lib, fn)(*args)
    return rc, last_error().decode() if rc else ""


# ---- the calls.  A template names the arguments the cases vary; everything else is fixed (pointers null unless a case needs them).
def fill(template, **kw):
    return " ".join(str(kw.get(t[1:], "?")) if t.startswith("$") else t for t in template.split(" "))


NULLS = lambda k: " ".join(["null"] * k)  # noqa: E731
PTRS = lambda k: " ".join(["ptr"] * k)  # noqa: E731
BEAM = {   # the five beam entry points: geometry(n, width, pitch) runs first, then the NULL test
    "init": "rc_search_init null $n 16 $cube $width null $pitch " + NULLS(6),
    "expand": "rc_search_expand null $n $width $pitch $cube " + NULLS(7),
    "select": "rc_search_select null null null $n $width $pitch $cube " + NULLS(9) + " 0 null",
    "advance": "rc_search_advance null null $n $width $pitch $cube " + NULLS(8) + " 5 null",
    "backtrack": "rc_search_backtrack null null $n $width $pitch $cube 5 null null null null",
}
# (n, width, pitch, cube): pitch 0, no multiple of 16, several tiles and no power of two, a tile below 512, the last power of two with
# S * pitch < 2^32 and the first beyond for both cubes, n and width out of range, too many candidates, the cube size, and one that passes
GEOMETRY = [(4, 2, 0, 3), (4, 2, 520, 3), (529, 1, 528, 3), (300, 1, 256, 3), (4, 2, 1 << 26, 3), (4, 2, 1 << 27, 3), (4, 2, 1 << 27, 2), (4, 2, 1 << 28, 2),
            (-1, 2, 512, 3), (0, 2, 512, 3), (4, 0, 512, 3), (4, 65537, 512, 3), (1 << 31, 32, 512, 3), (4, 2, 512, 4), (4, 2, 512, 3), (4, 2, 512, 2)]
PITCHES = [0, 520, 528, 256, 1 << 26, 1 << 27, 512]                     # as above, for a second tiled buffer of the 3x3x3

POOL = {   # pool_geometry(n, capacity, pool_pitch) of the A* entry points; rca_pop checks the beam's geometry(n, batch, pitch) first
    "init": "rca_init null $n 16 $cube $cap $ppitch " + NULLS(16) + " 0 null",
    "pop": "rca_pop $n $cube 2 $cap $ppitch " + NULLS(7) + " $pitch " + NULLS(6),
    "merge": "rca_merge $n $cube 2 $pitch $cap $ppitch $w " + NULLS(21) + " 0 null 0 null",
    "backtrack": "rca_backtrack $n $cube $cap null null null null null $len null",
}

# one-tile boundaries: the first pitch % 16 == 0 with rows * pitch >= 2^32 and the last one below it
EDGE = {rows: -(-(1 << 32) // rows // 16) * 16 for rows in (54, 24, 20, 7)}
for rows, p in EDGE.items():
    assert p % 16 == 0 and rows * p >= 1 << 32 > rows * (p - 16)

SYM_APPLY = "rcs_sym_apply $in $out $n $pin $pout $cube $sym $uniform null null"
SYM_CANON = "rcs_sym_canonical $in $n $pin $cube $symout $out $pout null"
NET = "rc_net_first_layer $code $n $pitch $cube $wt ptr $hidden $wfmt $act $out $ofmt $stride null"


def queries():
    for name, t in BEAM.items():
        for n, width, pitch, cube in GEOMETRY:
            yield fill(t, n=n, width=width, pitch=pitch, cube=cube)
    # own argument errors behind the NULL test, with every buffer the same aligned pointer: beam_in == beam_out stops the call
    yield "rc_search_advance ptr ptr 4 2 512 3 " + PTRS(8) + " 0 null"                  # max_depth < 1
    yield "rc_search_advance ptr odd 4 2 512 3 " + PTRS(8) + " 5 null"                  # beam_out misaligned (and overlapping)
    yield "rc_search_select " + PTRS(3) + " 1 1 512 3 " + PTRS(8) + " odd 0 null"       # workspace misaligned (and 0 bytes)
    for name, t in POOL.items():
        base = dict(n=4, cube=3, cap=8, ppitch=512, pitch=512, w="f:1.0", len=5)
        for ppitch in PITCHES:
            yield fill(t, **{**base, "ppitch": ppitch})
        for n, cap in ((0, 8), (4, 0), (1 << 16, 1 << 15), (1 << 31, 1)):
            yield fill(t, **{**base, "n": n, "cap": cap})
        yield fill(t, **{**base, "cube": 4})
        yield fill(t, **{**base, "cube": 2, "ppitch": 1 << 28})
    for pitch in PITCHES:
        yield fill(POOL["pop"], n=4, cube=3, cap=8, ppitch=512, pitch=pitch)
        yield fill(POOL["merge"], n=4, cube=3, cap=8, ppitch=512, pitch=pitch, w="f:1.0")
    for w in ("f:nan", "f:-1.0", "f:inf", "f:0.0"):
        yield fill(POOL["merge"], n=4, cube=3, cap=8, ppitch=512, pitch=512, w=w)
    for length in (0, -3):
        yield fill(POOL["backtrack"], n=4, cube=3, cap=8, len=length)
    # alignment: one odd pointer among aligned ones, the table size 0 stops the call
    yield "rca_init ptr 4 16 3 8 512 " + PTRS(7) + " odd " + PTRS(8) + " 0 null"
    yield "rca_merge 4 3 2 512 8 512 f:1.0 " + PTRS(10) + " odd " + PTRS(10) + " 0 ptr 0 null"

    # symmetries: pitch_in with out == NULL (apply: refused further down; canonical: sym_out == NULL), pitch_out with out == in
    for cube, rows in ((3, 54), (2, 24)):
        for pin, n in ((0, 4), (520, 4), (528, 529), (256, 300), (EDGE[rows], 4), (EDGE[rows] - 16, 4), (512, -1), (512, 4)):
            yield fill(SYM_APPLY, **{"in": "ptr", "out": "null", "n": n, "pin": pin, "pout": 512, "cube": cube, "sym": "null", "uniform": 0})
            yield fill(SYM_CANON, **{"in": "ptr", "out": "null", "n": n, "pin": pin, "pout": 512, "cube": cube, "symout": "null"})
        for pout, n in ((0, 4), (520, 4), (528, 529), (256, 300), (EDGE[rows], 4), (EDGE[rows] - 16, 4), (512, 4)):
            yield fill(SYM_APPLY, **{"in": "ptr", "out": "ptr", "n": n, "pin": 1024, "pout": pout, "cube": cube, "sym": "null", "uniform": 0})
            yield fill(SYM_CANON, **{"in": "ptr", "out": "ptr", "n": n, "pin": 1024, "pout": pout, "cube": cube, "symout": "null"})
    for inp, out in (("null", "null"), ("odd", "null"), ("ptr", "odd")):
        yield fill(SYM_APPLY, **{"in": inp, "out": out, "n": 4, "pin": 512, "pout": 0, "cube": 3, "sym": "null", "uniform": 0})
        yield fill(SYM_CANON, **{"in": inp, "out": out, "n": 4, "pin": 512, "pout": 0, "cube": 3, "symout": "null"})
    yield fill(SYM_APPLY, **{"in": "ptr", "out": "null", "n": 4, "pin": 512, "pout": 512, "cube": 4, "sym": "null", "uniform": 0})
    yield fill(SYM_CANON, **{"in": "ptr", "out": "null", "n": 4, "pin": 512, "pout": 512, "cube": 4, "symout": "null"})
    # behind the layout checks, at n == 0 with two distinct buffers: nothing can launch
    for sym, uniform in (("odd", 0), ("null", -1), ("null", 48), ("null", 24), ("null", 47)):
        yield fill(SYM_APPLY, **{"in": "ptr", "out": "ptr2", "n": 0, "pin": 512, "pout": 512, "cube": 3, "sym": sym, "uniform": uniform})
    yield fill(SYM_APPLY, **{"in": "ptr", "out": "ptr2", "n": 0, "pin": 512, "pout": 512, "cube": 2, "sym": "null", "uniform": 24})
    yield fill(SYM_CANON, **{"in": "ptr", "out": "null", "n": 0, "pin": 512, "pout": 512, "cube": 3, "symout": "odd"})

    # the net front: every layout case at n == 0
    base = dict(code="ptr", n=0, pitch=512, cube=3, wt="ptr", hidden=64, wfmt=4, act=0, out="ptr", ofmt=4, stride=64)
    for cube, rows in ((3, 20), (2, 7)):
        for pitch in (0, -16, 520, 528, 256, EDGE[rows], EDGE[rows] - 16):
            yield fill(NET, **{**base, "cube": cube, "pitch": pitch})
    for change in (dict(cube=4), dict(code="null"), dict(wt="null"), dict(out="null"), dict(n=-1, hidden=7), dict(hidden=7), dict(hidden=4104), dict(hidden=12), dict(wfmt=1),
                   dict(ofmt=2), dict(act=2), dict(stride=56), dict(code="odd"), dict(wt="odd"), dict(out="odd"), dict(ofmt=5, stride=68)):
        yield fill(NET, **{**base, **change})


def write(path):
    entries, seen = entry_points(), set()
    with open(path, "w") as f:
        for q in queries():
            assert "?" not in q, q
            if q not in seen:
                seen.add(q)
                rc, text = call(entries, q)
                f.write(f"{q}\t{rc}\t{text}\n")
    from rubiks_cube_solver_amd import _net_lib, _search_lib
    print(f"{path}: {len(seen)} calls, {os.path.getsize(path)} bytes from libraries {_search_lib.build_id()} / {_net_lib.build_id()}")


if __name__ == "__main__":
    write(os.path.join(HERE, "refusals.txt"))
