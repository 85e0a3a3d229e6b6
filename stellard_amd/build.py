"""In-tree build of every native artefact (no cmake, no JIT cache):

  stellard_amd/libstl.so         product: gfx950 kernels + C ABI (hipcc)
  tests/native/libhostemu.so     test harness: the device verify code compiled
                                 for the host (bound checks on)
  tests/native/libhostemu_keyset.so  the same for the keyset's comb code
  tests/native/libhostemu_keyset_map.so  the keyset's key -> index map
  tests/native/libhostemu_keycache.so  the decoded-key cache's check, hash and
                                 victim choice, and the workspace layout
  tests/native/libhostemu_keycache_alt.so  the cache's second-choice set and
                                 insert rule, and phase 1's split point half
  tests/native/libhostemu_signer.so  Hash160 and the signer kernel's per-row
                                 function
  tests/native/libhostemu_acctdir.so  the account directory's hash, probe,
                                 two-step insert and decision function
  tests/native/libhostemu_sigcache.so  the verified-ID cache's hash, probe
                                 and insert
  tests/native/libhostemu_shamap.so  the SHAMap root's nibble, common prefix,
                                 node rule and inner-node hash
  tests/native/libhostemu_shamap_tree.so  the resident SHAMap's bucket, delta,
                                 position and top rules and its staged apply
  tests/native/libhostemu_shamap_nodes.so  the stored inner nodes' masking,
                                 leaf and top rules and both staged calls
  tests/native/libhostemu_shamap_lookup.so  the resident SHAMap's in-bucket
                                 search, bucket-differs and rank rules and the
                                 staged lookup and compare
  tests/native/libhostemu_shamap_fork.so  the resident SHAMap's read clamp,
                                 the staged fork between trees of two
                                 capacities, the snapshot and the revert
  tests/native/libhostemu_shamap_fetch.so  the fetch pack's bucket, hasInnerNode
                                 and top rules and the staged call between
                                 generations of their trees' capacities
  tests/native/libhostemu_shamap_get.so  the rules of the answers by node ID
                                 (range, kind, FAT and PATH rows) and the
                                 staged call over a generation of its tree's size
  oracle/build/liboracle.so      test oracle: CPU restatement (make)
  oracle/_ref/libsodium_ref.so   test oracle: reference call path over libsodium

Usage: python -m stellard_amd.build [--product-only]
"""
import os
import shutil
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stellard_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")

PRODUCT_SRCS = ["stl_kernels.hip", "stl_keyset.hip", "stl_signer.hip", "stl_acctdir.hip", "stl_sigcache.hip",
                "stl_shamap.hip", "stl_shamap_tree.hip", "stl_shamap_lookup.hip", "stl_shamap_fetch.hip",
                "stl_shamap_get.hip", "stl_selftest.hip",
                "stl_api.cpp", "stl_api_keyset.cpp", "stl_api_authority.cpp", "stl_api_sigcache.cpp",
                "stl_api_shamap.cpp", "stl_api_shamap_tree.cpp", "stl_batcher.cpp"]
PRODUCT_DEPS = PRODUCT_SRCS + ["stl_kernels.h", "stl_verify_core.h", "stl_fe25519.h", "stl_ge25519.h",
                               "stl_sc25519.h", "stl_sha512.h", "stl_base_table.h", "stl_lattice.h", "stl_txblob.h", "stl_sign.h",
                               "stl_comb.h", "stl_keyset.h", "stl_keyset_map.h", "stl_keycache.h",
                               "stl_hash160.h", "stl_signer_core.h", "stl_signer.h",
                               "stl_acctdir_core.h", "stl_acctdir.h",
                               "stl_sigcache_core.h", "stl_sigcache.h",
                               "stl_shamap_core.h", "stl_shamap.h",
                               "stl_shamap_tree_core.h", "stl_shamap_tree.h",
                               "stl_shamap_lookup_core.h", "stl_shamap_lookup.h",
                               "stl_shamap_fetch_core.h", "stl_shamap_fetch.h",
                               "stl_shamap_get_core.h", "stl_shamap_get.h",
                               "stl_group.h", "stl_selftest.h", "stl_host.h",
                               os.path.join("..", "..", "include", "stl.h")]


def source_digest():
    """SHA-256 over the product's sources (PRODUCT_DEPS, in order): names the
    build a profile was taken on, and lets bench.py tell whether the committed
    profile summaries still describe the sources it runs."""
    import hashlib
    h = hashlib.sha256()
    for d in PRODUCT_DEPS:
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(os.path.basename(d).encode() + b"\0" + f.read())
    return h.hexdigest()


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd, cwd=ROOT):
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, cwd=cwd, check=True)


# per-object dependencies: the host sources see only the ABI header, the
# launcher declarations and their own shared header (HOST_ONLY: no kernel
# file includes it), so a host-side change does not recompile the kernels
# (about 100 s) -- the objects live in build/obj (git-ignored, never shipped)
HOST_ONLY = ["stl_host.h"]
HOST_DEPS = HOST_ONLY + ["stl_kernels.h", "stl_keyset.h", "stl_keyset_map.h", "stl_keycache.h", "stl_signer.h",
             "stl_acctdir.h", "stl_acctdir_core.h", "stl_sigcache.h", "stl_sigcache_core.h", "stl_shamap.h",
             "stl_shamap_tree.h", "stl_shamap_tree_core.h", "stl_shamap_lookup.h", "stl_shamap_fetch.h", "stl_shamap_get.h", "stl_shamap_core.h", "stl_sha512.h", os.path.join("..", "..", "include", "stl.h")]
OBJ_DIR = os.path.join(ROOT, "build", "obj")


def build_product(force=False, extra_flags=(), variant="variant"):
    out = os.path.join(ROOT, "stellard_amd", "libstl.so")
    deps = [os.path.join(CSRC, d) for d in PRODUCT_DEPS]
    if extra_flags:
        # variant builds (-D experiment switches): one command, nothing cached,
        # and never the product's path -- a variant written to libstl.so would
        # look newer than build/obj and survive the next default build (ADVICE
        # r5); load one with STL_LIB_PATH=build/ab/<variant>.so
        vout = os.path.join(ROOT, "build", "ab", variant + ".so")
        os.makedirs(os.path.dirname(vout), exist_ok=True)
        _run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", *extra_flags,
              "-o", vout] + [os.path.join(CSRC, s) for s in PRODUCT_SRCS])
        return vout
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = []
    for src in PRODUCT_SRCS:
        obj = os.path.join(OBJ_DIR, src + ".o")
        if src.endswith(".hip"):
            # each kernel file sees the headers, not the other sources: a change
            # to one leaves the other's object (and code objects) as they are
            sdeps = [d for d in deps
                     if not d.endswith((".hip", ".cpp", *HOST_ONLY)) or d.endswith(src)]
        else:
            sdeps = [os.path.join(CSRC, d) for d in [src] + HOST_DEPS]
        if force or _stale(obj, sdeps):
            _run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c", "-o", obj,
                  os.path.join(CSRC, src)])
        objs.append(obj)
    if force or _stale(out, objs):
        _run([HIPCC, f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", out] + objs)
    return out


def build_hostemu(force=False):
    out = os.path.join(ROOT, "tests", "native", "libhostemu.so")
    src = os.path.join(ROOT, "tests", "native", "hostemu.cpp")
    deps = [src] + [os.path.join(CSRC, d) for d in PRODUCT_DEPS]
    if force or _stale(out, deps):
        _run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, src])
    return out


def build_hostemu_keyset(force=False):
    out = os.path.join(ROOT, "tests", "native", "libhostemu_keyset.so")
    src = os.path.join(ROOT, "tests", "native", "hostemu_keyset.cpp")
    deps = [src] + [os.path.join(CSRC, d) for d in PRODUCT_DEPS]
    if force or _stale(out, deps):
        _run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, src])
    return out


# The quick host harnesses (a few seconds each): name -> (source, csrc deps).
SMALL_HARNESSES = {
    "keyset_map": ("hostemu_keyset_map.cpp", ("stl_keyset_map.h",)),
    "keycache": ("hostemu_keycache.cpp", ("stl_keycache.h", "stl_fe25519.h", "stl_ge25519.h", "stl_kernels.h")),
    "keycache_alt": ("hostemu_keycache_alt.cpp", ("stl_keycache.h", "stl_verify_core.h", "stl_fe25519.h",
                                                  "stl_ge25519.h", "stl_sc25519.h", "stl_lattice.h", "stl_sha512.h",
                                                  "stl_base_table.h")),
    "signer": ("hostemu_signer.cpp", ("stl_hash160.h", "stl_signer_core.h", "stl_txblob.h", "stl_sha512.h",
                                      "stl_fe25519.h")),
    "acctdir": ("hostemu_acctdir.cpp", ("stl_acctdir_core.h", "stl_hash160.h", "stl_signer_core.h", "stl_txblob.h",
                                        "stl_sha512.h", "stl_fe25519.h")),
    "sigcache": ("hostemu_sigcache.cpp", ("stl_sigcache_core.h",)),
    "shamap": ("hostemu_shamap.cpp", ("stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")),
    "shamap_tree": ("hostemu_shamap_tree.cpp", ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                "stl_fe25519.h")),
    "shamap_nodes": ("hostemu_shamap_nodes.cpp", ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                  "stl_fe25519.h")),
    "shamap_lookup": ("hostemu_shamap_lookup.cpp", ("stl_shamap_lookup_core.h", "stl_shamap_tree_core.h",
                                                    "stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")),
    "shamap_fork": ("hostemu_shamap_fork.cpp", ("stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                "stl_fe25519.h")),
    "shamap_fetch": ("hostemu_shamap_fetch.cpp", ("stl_shamap_fetch_core.h", "stl_shamap_lookup_core.h",
                                                  "stl_shamap_tree_core.h", "stl_shamap_core.h", "stl_sha512.h",
                                                  "stl_fe25519.h")),
    "shamap_get": ("hostemu_shamap_get.cpp", ("stl_shamap_get_core.h", "stl_shamap_fetch_core.h",
                                              "stl_shamap_lookup_core.h", "stl_shamap_tree_core.h",
                                              "stl_shamap_core.h", "stl_sha512.h", "stl_fe25519.h")),
}
_small_lock = threading.Lock()


def _small_out(name):
    return os.path.join(ROOT, "tests", "native", f"libhostemu_{name}.so")


def _build_small(name, force=False):
    """Builds one quick harness if stale, then any other quick harness whose
    library is absent: the test modules build theirs on load, each through
    its own entry below, except tests/sigcache_py.py as first committed, which
    only opens libhostemu_sigcache.so -- a tree whose tests/native lost its
    libraries after build() is whole again once any of them has loaded."""
    with _small_lock:
        for n in [name] + [m for m in SMALL_HARNESSES if m != name]:
            src, hdrs = SMALL_HARNESSES[n]
            src = os.path.join(ROOT, "tests", "native", src)
            out = _small_out(n)
            deps = [src] + [os.path.join(CSRC, h) for h in hdrs]
            if n == name and (force or _stale(out, deps)) or n != name and not os.path.exists(out):
                _run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, src])
    return _small_out(name)


def build_hostemu_keyset_map(force=False):
    return _build_small("keyset_map", force)


def build_hostemu_keycache(force=False):
    return _build_small("keycache", force)


def build_hostemu_keycache_alt(force=False):
    return _build_small("keycache_alt", force)


def build_hostemu_signer(force=False):
    return _build_small("signer", force)


def build_hostemu_acctdir(force=False):
    return _build_small("acctdir", force)


def build_hostemu_sigcache(force=False):
    return _build_small("sigcache", force)


def build_hostemu_shamap(force=False):
    return _build_small("shamap", force)


def build_hostemu_shamap_tree(force=False):
    return _build_small("shamap_tree", force)


def build_hostemu_shamap_nodes(force=False):
    return _build_small("shamap_nodes", force)


def build_hostemu_shamap_lookup(force=False):
    return _build_small("shamap_lookup", force)


def build_hostemu_shamap_fork(force=False):
    return _build_small("shamap_fork", force)


def build_hostemu_shamap_fetch(force=False):
    return _build_small("shamap_fetch", force)


def build_hostemu_shamap_get(force=False):
    return _build_small("shamap_get", force)


def build_oracle():
    oracle = os.path.join(ROOT, "oracle")
    targets = ["build/liboracle.so"]
    # the libsodium harness only builds where libsodium's headers exist
    if os.path.exists("/opt/conda/include/sodium.h"):
        targets.append("_ref/libsodium_ref.so")
    _run(["make", "-s", "-C", oracle] + targets)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    force = "--force" in argv
    if "--product-only" in argv:
        build_product(force=force)
        return
    # the product and the host harness are independent single-threaded
    # compiles of the same device code: run them side by side
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as ex:
        jobs = [ex.submit(build_product, force), ex.submit(build_hostemu, force),
                ex.submit(build_hostemu_keyset, force), ex.submit(build_hostemu_keyset_map, force),
                ex.submit(build_hostemu_keycache, force), ex.submit(build_hostemu_keycache_alt, force),
                ex.submit(build_hostemu_signer, force),
                ex.submit(build_hostemu_acctdir, force), ex.submit(build_hostemu_sigcache, force),
                ex.submit(build_hostemu_shamap, force), ex.submit(build_hostemu_shamap_tree, force),
                ex.submit(build_hostemu_shamap_nodes, force), ex.submit(build_hostemu_shamap_lookup, force),
                ex.submit(build_hostemu_shamap_fork, force), ex.submit(build_hostemu_shamap_fetch, force),
                ex.submit(build_hostemu_shamap_get, force)]
        for j in jobs:
            j.result()
    build_oracle()


if __name__ == "__main__":
    main()
