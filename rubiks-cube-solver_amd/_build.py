"""Build identity of the native libraries: a hash of the sources a library is compiled from, embedded at build time
(-DRC_SRC_HASH=..., returned by rc_build_id() / rc_tree_build_id() / rc_search_build_id() / rc_net_build_id()) and recomputed from the tree at load time.

A library whose embedded id differs from the tree's sources is STALE: __graft_entry__.build() recompiles it (it compares ids, not
mtimes -- touching the .so hides nothing) and _native.load() refuses to load it.  LIBRARIES below is the one description of the
libraries: the build and the loader both read it.  No torch import here: build() runs this before anything else is loaded."""
from __future__ import annotations

import hashlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
MARKER = b"rc-build-id:"                     # the id is stored in the binary as "rc-build-id:<16 hex digits>"

_HIPCC = ("hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17")
_GXX = ("g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-Wall", "-Wextra")


class Library:
    """One native library: what it is compiled from and how, its override variable, how a process asks it who it is.  To add a
    library: one row in LIBRARIES here, and a binding module with its signature table (SIGNATURES, build_id(); see _native.load)."""

    def __init__(self, name, binding, file, sources, toolchain, env, id_symbol, error_symbol, headers=()):
        self.name, self.binding, self.file, self.toolchain, self.env = name, binding, file, toolchain, env   # binding: its ctypes module
        self.gpu = toolchain is _HIPCC                                              # device code: loaded after torch, to share its HIP runtime
        self.id_symbol, self.error_symbol = id_symbol, error_symbol                 # error_symbol None: the library keeps no last error
        # every file the id hashes, in this order (source_hash depends on it): the translation unit that is compiled and the
        # headers it includes from csrc/, then the public header in include/, then `headers`: further public headers of include/
        # (an extension of the library with a header of its own, e.g. rubikepisode.h)
        self.sources = (*(os.path.join(_HERE, "csrc", s) for s in sources[:-1]), *(os.path.join(_ROOT, "include", h) for h in (sources[-1], *headers)))
        self.built = os.path.join(_HERE, file)                                      # where build() writes it, whatever `env` says

    def command(self, src_id, out):
        """The one compile line of each toolchain.  The id hashes the sources only: to fold the flags in, hash this list too."""
        return [*self.toolchain, "-fPIC", "-shared", f"-DRC_SRC_HASH={src_id}", self.sources[0], "-o", out]


LIBRARIES = {l.name: l for l in (
    Library("hip", "_lib", "librubikhip.so", ("rubikhip.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h", "rc_cubies.h", "rc_edge.h", "rc_chain.h", "rc_ida.h",
                                              "rc_episode.h", "rubikhip.h"), _HIPCC, "RUBIKHIP_LIB", "rc_build_id", "rc_last_error", headers=("rubikepisode.h",)),
    Library("tree", "_tree", "librubiktree.so", ("rc_tree.cpp", "rc_host.h", "rubiktree.h"), _GXX, "RUBIKTREE_LIB", "rc_tree_build_id", None),
    Library("search", "_search_lib", "librubiksearch.so", ("rc_search.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h", "rc_sym.h", "rc_sym_tables.h", "rubiksearch.h"),
            _HIPCC, "RUBIKSEARCH_LIB", "rc_search_build_id", "rc_search_last_error", headers=("rubiksym.h",)),
    Library("net", "_net_lib", "librubiknet.so", ("rc_net.hip", "rc_host.h", "rubiknet.h"), _HIPCC, "RUBIKNET_LIB", "rc_net_build_id", "rc_net_last_error"))}
HIP_SOURCES, TREE_SOURCES, SEARCH_SOURCES, NET_SOURCES = (LIBRARIES[n].sources for n in ("hip", "tree", "search", "net"))


def source_hash(paths) -> str | None:
    """sha256 over (file name, length, bytes) of every source, first 16 hex digits; None if a source is absent (an installed copy
    without its sources cannot be checked)."""
    h = hashlib.sha256()
    for p in paths:
        if not os.path.exists(p):
            return None
        data = open(p, "rb").read()
        h.update(os.path.basename(p).encode() + b"\0" + str(len(data)).encode() + b"\0" + data)
    return h.hexdigest()[:16]


def embedded_id(lib_path) -> str | None:
    """The id stored in a built library, read from the file's bytes (no dlopen: build() must be able to replace the file)."""
    if not os.path.exists(lib_path):
        return None
    data = open(lib_path, "rb").read()
    i = data.find(MARKER)
    if i < 0:
        return None
    return data[i + len(MARKER):i + len(MARKER) + 16].decode("ascii", "replace")


def check_loaded(name, reported: str, paths):
    """Raise if the id a LOADED library reports is not the hash of the sources in this tree (RC_ALLOW_STALE=1 turns it into a pass:
    A/B experiments that load an older build through RUBIKHIP_LIB)."""
    want = source_hash(paths)
    if want is None or reported == want or os.environ.get("RC_ALLOW_STALE") == "1":
        return
    raise RuntimeError(f"{name} is stale: it was built from sources with id {reported!r}, the tree's sources have id {want!r}; rebuild with "
                       "`python -c 'import __graft_entry__ as g; g.build()'`")
