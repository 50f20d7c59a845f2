"""Case tables of the layout tests (tests/test_gpu_layouts.py on the device, tests/test_layouts_host.py on the CPU).

include/rubikhip.h gives every operand of an entry point a tiling of its own (pitch_in / pitch_out / code_pitch / act_pitch).  The
tests here give every operand a DIFFERENT one, so that a kernel which addressed one operand with another operand's pitch or tile
shift computes something else than the oracle.

Layouts of a buffer that holds n cubes (ceil16(n) = n rounded up to a multiple of 16):

    name     pitch                tiles
    tight    ceil16(n)            1
    padded   ceil16(n) + 48       1      (not a power of two)
    t512     512                  ceil(n / 512)
    t1024    1024                 ceil(n / 1024)

Sizes 513, 1029, 2565: whole 512-cube wave spans plus a ragged tail of 1 or 5 cubes, so the FULL path and the tail path of the packed
kernels both run for pack widths 1 and 2, and every wave of pack width 2 opens a new 512 tile.  t512 has several tiles at every size;
t1024 has one tile at n = 513 (there it is a third one-tile pitch, 1024) and several from 1029 on.

Exclusions: none.  The pitches of the four layouts differ from each other at every size of the table (528 / 576 / 512 / 1024,
1040 / 1088 / 512 / 1024, 2576 / 2624 / 512 / 1024), and tests/test_layouts_host.py::test_teeth proves for every ordered pair and
size that states scattered under one layout and gathered under the other come back different.
"""
import itertools

LAYOUTS = ("tight", "padded", "t512", "t1024")
SIZES = (513, 1029, 2565)
CUBE_SIZES = (3, 2)
S_OF = {2: 24, 3: 54}
A_OF = {2: 6, 3: 12}
SL_OF = {2: 7, 3: 20}
NF_OF = {2: 15, 3: 51}
RC_OF = {2: (7, 21), 3: (20, 24)}
DENSE = ("U8", "F16", "BF16", "F32")
EXCLUDED = {}                      # (X, Y) -> sizes at which the pair has no teeth; empty, see the module docstring


def ceil16(n):
    return -(-n // 16) * 16


def layout(name, n):
    """-> (pitch, tiles)"""
    if name == "tight":
        return ceil16(n), 1
    if name == "padded":
        return ceil16(n) + 48, 1
    pitch = {"t512": 512, "t1024": 1024}[name]
    return pitch, -(-n // pitch)


def shape(name, n, rows):
    pitch, tiles = layout(name, n)
    return tiles, rows, pitch


def check_premise(n, *names):
    """What a case claims about its layouts: distinct names are distinct pitches, the tile counts are the table's, t512 always has
    several tiles and t1024 has them as soon as n > 1024."""
    for x, y in itertools.combinations(set(names), 2):
        assert layout(x, n)[0] != layout(y, n)[0], (x, y, n)
    for x in names:
        pitch, tiles = layout(x, n)
        assert pitch % 16 == 0 and pitch * tiles >= n
        if x in ("tight", "padded"):
            assert tiles == 1 and pitch >= n and pitch & (pitch - 1)            # one tile, not a power of two
        else:
            assert tiles == -(-n // pitch) and (tiles > 1) == (n > pitch)
    assert layout("t512", n)[1] > 1
    if any(x == "t1024" for x in names) and n > 1024:
        assert layout("t1024", n)[1] > 1


def all_differ(n, *names):
    return len({layout(x, n)[0] for x in names}) == len(names)


# ------------------------------------------------------------------------------------------------- the header's address rule
def address(cube, row, pitch, rows):
    """include/rubikhip.h "State layout": st[(n / pitch) * S * pitch + s * pitch + n % pitch]."""
    return (cube // pitch) * rows * pitch + row * pitch + cube % pitch


def scatter(aos, pitch, tiles, size=None):
    """[n, rows] -> flat byte list laid out by the rule, one element at a time."""
    n, rows = len(aos), len(aos[0])
    flat = [0] * max(tiles * rows * pitch, size or 0)
    for c in range(n):
        for r in range(rows):
            flat[address(c, r, pitch, rows)] = int(aos[c][r])
    return flat


def gather(flat, n, rows, pitch):
    return [[flat[address(c, r, pitch, rows)] for r in range(rows)] for c in range(n)]


def nbytes(name, n, rows):
    pitch, tiles = layout(name, n)
    return tiles * rows * pitch


# ------------------------------------------------------------------------------------------------- section A: the case generators
PAIRS = tuple(itertools.product(LAYOUTS, LAYOUTS))                 # every ordered pair, equal ones included
TRIPLES = tuple(itertools.product(LAYOUTS, LAYOUTS, LAYOUTS))
POLICY_TRIPLE = ("t512", "padded", "t1024")                        # in, out, code: three different layouts at every size
STEP_POLICIES = (1, 2, 3, 4)                                       # RC_VARIANT_STEP_POLICY: every value besides the default 0


def step_code_cases():
    """rc_apply_moves_ex with the compact code -> (in, out, code, variant, in_place)."""
    out = []
    for pack in (1, 2):
        for li, lo, lc in TRIPLES:
            out.append((li, lo, lc, pack, False))
        for li in LAYOUTS:
            for lc in LAYOUTS:
                if lc != li:
                    out.append((li, li, lc, pack, True))
        for pol in STEP_POLICIES:
            out.append((*POLICY_TRIPLE, pol * 10 + pack, False))
    return out


def step_dense_cases():
    """rc_apply_moves_ex with a dense one-hot -> (in, out, variant); the format is the test's parameter."""
    return [(li, lo, tile * 100000) for tile in (1, 2) for li, lo in PAIRS]


WORKSPACE_CASE = dict(cs=3, fmt="BF16", n=(1 << 17) + 5, lin="t512", lout="tight")


def encode_cases():
    """rc_encode / rc_is_solved -> (state layout, output): output = a code layout, a dense format name or "flags"."""
    return ([(ls, lc) for ls, lc in PAIRS] + [(ls, f) for ls in LAYOUTS for f in DENSE] + [(ls, "flags") for ls in LAYOUTS])


EXPAND_PARTS = (1, 3, "A")
EXPAND_OUTPUTS = {"all": (True, True, True), "flags": (False, True, False), "stickers": (True, True, False)}   # children, flags, codes


def expand_cases():
    """rc_expand_children_ex -> (in, out tiling, variant without the parts field, parts, outputs).
    Streaming form excluded (RC_VARIANT_EXPAND_STREAM(8)): pack 1 / 2 x parts 1 / 3 / A x (children + codes + flags | flags alone).
    Streaming form forced (RC_VARIANT_EXPAND_STREAM(1)): the launcher only takes it for children without codes, with no parts field
    and a pack that is not 1 (expand_stream_grid), so those cases write children + flags with pack 0 (default) and 2."""
    out = []
    for li, lo in PAIRS:
        for pack in (1, 2):
            for parts in EXPAND_PARTS:
                for outputs in ("all", "flags"):
                    out.append((li, lo, pack + 800, parts, outputs))
        for pack in (0, 2):
            out.append((li, lo, pack + 100, None, "stickers"))
    return out


def expand_variant(base, parts, A):
    return base + 1000 * (0 if parts is None else A if parts == "A" else parts)


# rc_onehot_from_code_ex: check_variant(RC_OP_CODE_TO_DENSE) accepts the same fields for both cube sizes -- forms 1 and 2 alone, form 3
# with a skew (tens) and a group count (thousands), forms 0 and 4 with fronts 1 / 2 / 4 (units) and fetch 2 / 3 / 4 (tens)
DENSE_FORMS = ((100000, 200000, 300000, 300000 + 1000 * 2 + 10 * 3, 400000) +
               tuple(400000 + f + 10 * t for f in (1, 2, 4) for t in (2, 3, 4)) +
               tuple(400000 + f for f in (1, 2, 4)) + tuple(400000 + 10 * t for t in (2, 3, 4)) + (0, 4 + 10 * 4))


def code_to_dense_cases():
    """-> (code layout, variant); the format is the test's parameter."""
    return [(lc, v) for lc in LAYOUTS for v in DENSE_FORMS]


SCRAMBLE_MODES = ("replay", "drawn", "copy")


def scramble_cases(n):
    """rc_scramble / rc_scramble_from -> (state layout, act_pitch, mode, from_src)."""
    return [(ls, ap, mode, src) for ls in LAYOUTS for ap in (ceil16(n), ceil16(n) + 32) for mode in SCRAMBLE_MODES for src in (False, True)]


# ------------------------------------------------------------------------------------------------- section B: carved operands
def carve_offsets(count):
    """16, 48, 80, ...: every operand 16 bytes past a 32-byte boundary, no two with the same phase within 256 bytes (count <= 8);
    beyond eight operands the phases repeat."""
    return [16 + 32 * (i % 8) for i in range(count)]
