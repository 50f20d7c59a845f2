"""The plumbing every native library shares (_build.LIBRARIES, _native.load, __graft_entry__.build_library), once per library and
without a GPU: header <-> exports <-> signature table, the build id, the refusal of a stale or missing library, the build's temporary file."""
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# library -> (its public header, the rc_* names where a set is pinned exactly, how many there are)
LIBS = {
    "hip": ("rubikhip.h", None, 38),
    "tree": ("rubiktree.h", None, 12),
    "search": ("rubiksearch.h", {"rc_search_build_id", "rc_search_last_error", "rc_search_workspace_bytes", "rc_search_init", "rc_search_expand",
                                 "rc_search_select", "rc_search_advance", "rc_search_backtrack"}, 8),
    "net": ("rubiknet.h", {"rc_net_build_id", "rc_net_last_error", "rc_net_first_layer"}, 3),
}
HIP_NAMES = {"rc_build_id", "rc_onehot_from_code_blocks", "rc_describe_dispatch", "rc_facade_release", "rc_apply_moves_ws", "rc_encode_ws", "rc_workspace_bytes",
             "rc_adi_generate_family", "rc_family_layout", "rc_onehot_from_family", "rc_onehot_from_family_depths", "rc_adi_targets_depths",
             "rc_legacy_scramble_actions_ex", "rc_host_alias", "rc_scramble_from", "rc_search_pack"}


def binding(name):
    from rubiks_cube_solver_amd import _build
    return importlib.import_module("rubiks_cube_solver_amd." + _build.LIBRARIES[name].binding)


def prototypes(header):
    """{function: number of parameters} of every rc_* prototype of a public header, comments stripped, (void) = 0."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t|const char \*|void|rc_tree \*)\s*(rc_\w+)\(([^)]*)\)", text, re.M)
    return {fn: 0 if args.strip() in ("", "void") else args.count(",") + 1 for fn, args in found}


@pytest.mark.parametrize("name", LIBS)
def test_header_exports_and_signature_table_agree(name):
    """What the header declares = what the .so exports (every rc_*, and nothing else leaves it) = what the signature table names, with
    as many argument types as the prototype has parameters; the binary is the tree's sources."""
    from rubiks_cube_solver_amd import _build, _native
    mod, (header, pinned, count) = binding(name), LIBS[name]
    L = _native.load(name, mod.SIGNATURES)                              # loads without a GPU
    spec, protos = _build.LIBRARIES[name], prototypes(header)
    assert set(LIBS) == set(_build.LIBRARIES)                           # a new row in the table needs its row here
    declared = set(protos)
    assert len(declared) == count and (pinned is None or declared == pinned) and (name != "hip" or HIP_NAMES <= declared), declared
    assert {spec.id_symbol, *([spec.error_symbol] if spec.error_symbol else [])} <= declared
    for fn in declared:
        assert hasattr(L, fn), fn
    nm = subprocess.run(["nm", "-D", "--defined-only", mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert {e for e in exported if e.startswith("rc_")} == declared, exported ^ declared
    assert set(mod.SIGNATURES) == declared, set(mod.SIGNATURES) ^ declared
    for fn, n_params in protos.items():
        assert len(_native.signature(mod.SIGNATURES[fn])[0]) == n_params, fn
    # the id embedded at build time = the hash of the library's sources as they are on disk (a stale library would not even have loaded)
    assert mod.build_id() == _build.source_hash(spec.sources) == _build.embedded_id(mod.LIB_PATH) and len(mod.build_id()) == 16
    assert os.path.exists(os.path.join(ROOT, "rubiks-cube-solver_amd", spec.file))


@pytest.mark.parametrize("name", LIBS)
def test_a_stale_or_missing_library_is_refused(tmp_path, name):
    """The binding loads only a library whose embedded source hash equals the hash of the tree's sources; modification times decide
    nothing.  A copy of the shipped library with ONE hex digit of its id changed (= a binary built from other sources) and the newest
    mtime of all: refused in a fresh process, accepted only with RC_ALLOW_STALE=1 (A/B experiments), and seen as stale by the
    build's own check.  A missing library says how to build it."""
    from rubiks_cube_solver_amd import _build
    mod, spec = binding(name), _build.LIBRARIES[name]
    want = _build.source_hash(spec.sources)
    assert want and _build.embedded_id(mod.LIB_PATH) == want
    fake = str(tmp_path / spec.file)
    data = bytearray(open(mod.LIB_PATH, "rb").read())
    i = data.find(_build.MARKER) + len(_build.MARKER)
    data[i] = ord("0") if data[i] != ord("0") else ord("1")
    open(fake, "wb").write(bytes(data))
    os.utime(fake, None)                                               # newer than every source: an mtime rule would call it current
    assert _build.embedded_id(fake) != want and os.path.getmtime(fake) >= max(os.path.getmtime(p) for p in spec.sources)
    code = f"from rubiks_cube_solver_amd import {spec.binding} as m; print('loaded', m.build_id())"
    env = dict(os.environ, **{spec.env: fake})
    env.pop("RC_ALLOW_STALE", None)
    run = lambda env: subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    out = run(env)
    assert out.returncode != 0 and "is stale" in out.stderr and "loaded" not in out.stdout, out.stderr[-2000:]
    out = run(dict(env, RC_ALLOW_STALE="1"))
    assert out.returncode == 0 and "loaded " + _build.embedded_id(fake) in out.stdout, out.stderr[-2000:]
    out = run(dict(env, **{spec.env: str(tmp_path / "missing.so")}))
    assert out.returncode != 0 and "not found" in out.stderr and "loaded" not in out.stdout, out.stderr[-2000:]
    # a library without any id (built by hand without -DRC_SRC_HASH, or one that predates the id) is stale too
    plain = str(tmp_path / "no_id.so")
    open(plain, "wb").write(b"\x7fELF" + b"\0" * 64)
    assert _build.embedded_id(plain) is None and _build.embedded_id(str(tmp_path / "missing.so")) is None


def test_build_compiles_into_a_temporary_file_of_its_own(tmp_path, monkeypatch):
    """build_library compiles into <library>.<pid>.so.tmp next to the library (two builds at once cannot delete or rename each
    other's output) and leaves no temporary file behind; a failed compile leaves the existing library as it was.  The compiler is a
    stub here, and the library a copy in tmp_path."""
    import __graft_entry__ as g
    b = g._build_mod()
    spec = b.LIBRARIES["tree"]
    lib = str(tmp_path / spec.file)
    shutil.copy(spec.built, lib)
    before = open(lib, "rb").read()
    spec.built = lib
    monkeypatch.setattr(g, "_build_mod", lambda: b)
    seen = []

    def compiler(cmd, fail=False):
        out = cmd[cmd.index("-o") + 1]
        seen.append(out)
        open(out, "wb").write(b"half" if fail else before + b"new")
        if fail:
            raise subprocess.CalledProcessError(1, cmd)
    monkeypatch.setattr(g.subprocess, "check_call", compiler)
    assert g.build_library("tree", force=True) == lib
    monkeypatch.setattr(g.subprocess, "check_call", lambda cmd: compiler(cmd, fail=True))
    with pytest.raises(subprocess.CalledProcessError):
        g.build_library("tree", force=True)
    assert len(seen) == 2 and open(lib, "rb").read() == before + b"new" and os.listdir(tmp_path) == [spec.file]
    for tmp in seen:
        assert os.path.dirname(tmp) == str(tmp_path) and tmp.endswith(".so.tmp") and tmp != lib + ".tmp" and f".{os.getpid()}." in os.path.basename(tmp)
