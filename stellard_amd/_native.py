"""ctypes binding of libstl.so (the C ABI in include/stl.h).

The shared library is built in-tree by ``stellard_amd.build`` (hipcc,
--offload-arch=gfx950).  There is no Python or CPU fallback: if the library is
missing this module raises, so a GPU run can never silently verify on the host.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STL_LIB_PATH") or os.path.join(_HERE, "libstl.so")

STL_OK = 0
STL_EINVAL = -22
STL_ENODEV = -19
STL_ENOMEM = -12
STL_EHIP = -1000
STL_ERCCL = -1001

# stl_config.flags
STL_CFG_RCCL_GATHER = 0x1
STL_CFG_NO_RCCL = 0x2

# signed-object kinds of the blob entry points
STL_BLOB_TRANSACTION = 0
STL_BLOB_VALIDATION = 1

STL_POLICY_SODIUM_1_0_18 = 0x0
STL_POLICY_STELLARD_1_0_0 = 0x1
STL_POLICY_MASK = 0x1
STL_REQUIRE_S_LT_L = 0x2
STL_FULL_LENGTH = 0x4
STL_DEDUP_KEYS = 0x8
STL_ONE_LANE = 0x10
STL_NO_AUTO_DEDUP = 0x20
STL_DEBUG_RAW_PREDICATE = 0x80000000  # test-only: no S < L (stl.h)

# registered signer sets (stl_keyset_*)
STL_KEYSET_MAX_KEYS = 4096
STL_KEYSET_BASE = 0xFFFFFFFF
STL_KEYSET_NOT_FOUND = 0xFFFFFFFF

# stl_debug_tuning keys
STL_TUNE_FUSED_PREP = 0
STL_TUNE_MAIN_QUEUE = 1
STL_TUNE_STREAMS = 2
STL_TUNE_CHUNK_LOG2 = 3
STL_TUNE_BYTE_SHARDS = 4
STL_TUNE_QUAD = 5
STL_TUNE_STREAM_WORKSPACES = 6
STL_TUNE_RCCL_TIMEOUT_MS = 7
STL_TUNE_LONG_HASH = 8
STL_TUNE_SHARED_KEYS = 9
STL_TUNE_WIDE_MIN_ROWS = 10
STL_TUNE_R_AHEAD = 11
STL_TUNE_FIRST_CHUNK = 12
STL_TUNE_KEY_CACHE = 13
STL_TUNE_SHAMAP_LOOKUP_BUCKETS = 14

# per-transaction status of the serialized-transaction entry points
STL_TX_OK = 0
STL_TX_DEFERRED = 1
STL_TX_MALFORMED = 2

# signer authority (stl_account_id_batch*, stl_tx_blob_signer_batch*)
STL_ACCOUNT_ID_BYTES = 20
STL_SIGNER_NOT_MASTER = 0
STL_SIGNER_MASTER = 1
STL_SIGNER_UNDECIDED = 2

# account directory (stl_acctdir_*)
STL_ACCT_HAS_REGULAR_KEY = 0x1
STL_ACCT_MASTER_DISABLED = 0x2
STL_ACCT_ABSENT = 0x4
STL_ACCT_NOT_FOUND = 0xFF
STL_ACCTDIR_MAX_ACCOUNTS = 16777216
STL_AUTH_MASTER = 0
STL_AUTH_REGULAR = 1
STL_AUTH_MASTER_DISABLED = 2
STL_AUTH_BAD_AUTH = 3
STL_AUTH_BAD_AUTH_MASTER = 4
STL_AUTH_NO_ACCOUNT = 5
STL_AUTH_UNDECIDED = 6

# verified-ID cache (stl_sigcache_*)
STL_SIGCACHE_MAX_SETS_LOG2 = 24
STL_SIGCACHE_WAYS = 4

# SHAMap root (stl_shamap_root*)
STL_SHAMAP_MAX_ITEMS = 16777216

# SHAMap inner nodes (stl_shamap_nodes*, stl_shamap_tree_apply_nodes*)
STL_SHAMAP_MAX_NODES = 0xFFFFFFC0
STL_SHAMAP_NODE_BODY_BYTES = 512

# resident SHAMap compare (stl_shamap_tree_compare*)
STL_SHAMAP_DIFF_A_ONLY = 1
STL_SHAMAP_DIFF_B_ONLY = 2
STL_SHAMAP_DIFF_CHANGED = 3

# resident SHAMap nodes by node ID and paths by key (stl_shamap_tree_get_nodes*)
STL_SHAMAP_GET_MAX_REQUESTS = 16777216
STL_SHAMAP_GET_NODE = 0
STL_SHAMAP_GET_FAT = 1
STL_SHAMAP_GET_PATH = 2
STL_SHAMAP_AT_ABSENT = 0
STL_SHAMAP_AT_INNER = 1
STL_SHAMAP_AT_LEAF = 2
STL_SHAMAP_AT_EMPTY_ROOT = 3
STL_SHAMAP_AT_INVALID = 4
STL_SHAMAP_AT_OTHER_LEAF = 5

# arithmetic self-test (stl_debug_selftest_*; row formats in csrc/stl_selftest.h)
STL_SELFTEST_OPS = 47
STL_SELFTEST_GROUP_OPS = 7
STL_SELFTEST_IN_WORDS = 72
STL_SELFTEST_OUT_WORDS = 40
STL_SELFTEST_MAX_ROWS = 1048576

# Every entry point include/stl.h declares: (name, restype, argtypes)
_P = ctypes.c_void_p
_U8P = ctypes.c_void_p
SYMBOLS = [
    ("stl_init", ctypes.c_int, [_P]),
    ("stl_shutdown", None, []),
    ("stl_device_count", ctypes.c_int, []),
    ("stl_version", ctypes.c_char_p, []),
    ("stl_strerror", ctypes.c_char_p, [ctypes.c_int]),
    ("stl_ed25519_verify_detached", ctypes.c_int, [_U8P, _U8P, ctypes.c_ulonglong, _U8P]),
    ("stl_ed25519_verify_batch", ctypes.c_int, [_U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, ctypes.c_uint32]),
    ("stl_tx_verify_batch", ctypes.c_int,
     [_U8P, _P, _P, _U8P, _U8P, ctypes.c_size_t, _U8P, ctypes.c_uint32]),
    ("stl_ed25519_verify_batch_device", ctypes.c_int,
     [_U8P, _U8P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P]),
    ("stl_tx_hash_batch_device", ctypes.c_int, [_U8P, _P, _P, ctypes.c_size_t, _U8P, _P]),
    ("stl_ed25519_sign_batch_device", ctypes.c_int, [_U8P, _U8P, ctypes.c_size_t, _U8P, _U8P, _P]),
    ("stl_tx_blob_verify_batch", ctypes.c_int,
     [_U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, ctypes.c_uint32]),
    ("stl_tx_blob_prepare_device", ctypes.c_int,
     [_U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, _U8P, _U8P, _P]),
    ("stl_tx_verify_batch_device", ctypes.c_int,
     [_U8P, _P, _P, _U8P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P]),
    ("stl_signed_blob_verify_batch_device", ctypes.c_int,
     [ctypes.c_uint32, _U8P, _P, _P, ctypes.c_size_t, _P, _U8P, _U8P, ctypes.c_uint32, _P]),
    ("stl_batcher_create", ctypes.c_void_p, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    ("stl_batcher_submit", ctypes.c_int, [_P, _U8P, _U8P, _U8P, _P, _P]),
    ("stl_batcher_submit_tx", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _P, _P]),
    ("stl_batcher_flush", None, [_P]),
    ("stl_batcher_stats", None, [_P, _P, _P, _P]),
    ("stl_batcher_destroy", None, [_P]),
    ("stl_signed_blob_verify_batch", ctypes.c_int,
     [ctypes.c_uint32, _U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, ctypes.c_uint32]),
    ("stl_signed_blob_prepare_device", ctypes.c_int,
     [ctypes.c_uint32, _U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, _U8P, _U8P, _P]),
    ("stl_comm_unique_id", ctypes.c_int, [_U8P]),
    ("stl_comm_init_rank", ctypes.c_int, [ctypes.c_int, ctypes.c_int, _U8P]),
    ("stl_comm_destroy", None, []),
    ("stl_comm_abort", None, []),
    ("stl_comm_sync", ctypes.c_int, [_P, ctypes.c_int]),
    ("stl_comm_info", ctypes.c_int, [_P, _P]),
    ("stl_bitmap_gather_device", ctypes.c_int, [_P, ctypes.c_size_t, _P, ctypes.c_int, _P]),
    ("stl_bitmap_gatherv_device", ctypes.c_int, [_P, ctypes.c_size_t, _P, _P, ctypes.c_int, _P]),
    ("stl_shard_range", None, [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _P, _P]),
    ("stl_shard_range_bytes", None, [_P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _P, _P]),
    ("stl_debug_fault_after", None, [ctypes.c_longlong]),
    ("stl_get_stats", ctypes.c_int, [_P]),
    ("stl_reset_stats", None, []),
    ("stl_set_phase_timing", ctypes.c_int, [ctypes.c_int]),
    ("stl_debug_verify_k_device", ctypes.c_int, [_U8P, _U8P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P]),
    ("stl_debug_tuning", ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    ("stl_debug_stream_contexts", ctypes.c_int, []),
    ("stl_debug_key_cache_clear", ctypes.c_int, []),
    ("stl_debug_key_cache_info", ctypes.c_int, [_P, _P, _P, _P]),
    ("stl_debug_clock_stamp", ctypes.c_int, [_P, ctypes.c_uint32, _P]),
    ("stl_debug_selftest_ops_device", ctypes.c_int, [ctypes.c_uint32, _P, ctypes.c_size_t, _P, _P]),
    ("stl_debug_selftest_group_device", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_size_t, _P, _P]),
    ("stl_release_stream", ctypes.c_int, [_P]),
    ("stl_debug_sign_adversarial_device", ctypes.c_int,
     [_U8P, _U8P, _U8P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, _P]),
    ("stl_keyset_create", ctypes.c_int, [_U8P, ctypes.c_size_t, ctypes.c_uint32, _P]),
    ("stl_keyset_destroy", None, [_P]),
    ("stl_keyset_get_info", ctypes.c_int, [_P, _P]),
    ("stl_keyset_find", ctypes.c_longlong, [_P, _U8P]),
    ("stl_keyset_verify_batch", ctypes.c_int, [_P, _P, _U8P, _U8P, ctypes.c_size_t, _U8P, ctypes.c_uint32]),
    ("stl_keyset_verify_batch_device", ctypes.c_int,
     [_P, _P, _U8P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P]),
    ("stl_keyset_tx_verify_batch_device", ctypes.c_int,
     [_P, _P, _U8P, _P, _P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P]),
    ("stl_debug_keyset_rows", ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P]),
    ("stl_keyset_lookup_device", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _P, _P, _P]),
    ("stl_keyset_verify_by_key_device", ctypes.c_int,
     [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _P, ctypes.c_uint32, _P, _P]),
    ("stl_keyset_verify_by_key", ctypes.c_int, [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, ctypes.c_uint32]),
    ("stl_keyset_signed_blob_verify_batch_device", ctypes.c_int,
     [_P, ctypes.c_uint32, _U8P, _P, _P, ctypes.c_size_t, _P, _U8P, _U8P, ctypes.c_uint32, _P, _P]),
    ("stl_account_id_batch", ctypes.c_int, [_U8P, ctypes.c_size_t, _U8P]),
    ("stl_account_id_batch_device", ctypes.c_int, [_U8P, ctypes.c_size_t, _U8P, _P]),
    ("stl_tx_blob_signer_batch_device", ctypes.c_int, [_U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, _P]),
    ("stl_tx_blob_signer_batch", ctypes.c_int, [_U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P]),
    ("stl_acctdir_create", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint64, _P]),
    ("stl_acctdir_destroy", None, [_P]),
    ("stl_acctdir_get_info", ctypes.c_int, [_P, _P]),
    ("stl_acctdir_upsert", ctypes.c_int, [_P, _U8P, _U8P, _U8P, ctypes.c_size_t]),
    ("stl_acctdir_lookup_device", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _U8P, _U8P, _P]),
    ("stl_acctdir_tx_blob_authority_device", ctypes.c_int,
     [_P, _U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, _P]),
    ("stl_acctdir_tx_blob_authority", ctypes.c_int, [_P, _U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P]),
    ("stl_sigcache_create", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, _P]),
    ("stl_sigcache_destroy", None, [_P]),
    ("stl_sigcache_get_info", ctypes.c_int, [_P, _P]),
    ("stl_sigcache_clear", ctypes.c_int, [_P, _P]),
    ("stl_sigcache_lookup_device", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _P, _P]),
    ("stl_sigcache_signed_blob_verify_batch_device", ctypes.c_int,
     [_P, _U8P, _P, _P, ctypes.c_size_t, _P, _U8P, _U8P, ctypes.c_uint32, _P, _P, _P]),
    ("stl_sigcache_signed_blob_verify_batch", ctypes.c_int,
     [_P, _U8P, _P, _P, ctypes.c_size_t, _U8P, _U8P, _U8P, ctypes.c_uint32, _P, _P]),
    ("stl_shamap_root_device", ctypes.c_int, [_U8P, _U8P, _P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_root", ctypes.c_int, [_U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P]),
    ("stl_shamap_tree_create", ctypes.c_int, [ctypes.c_uint32, _P]),
    ("stl_shamap_tree_destroy", None, [_P]),
    ("stl_shamap_tree_get_info", ctypes.c_int, [_P, _P]),
    ("stl_shamap_tree_apply_device", ctypes.c_int, [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_tree_apply", ctypes.c_int, [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P]),
    ("stl_shamap_tree_root_device", ctypes.c_int, [_P, _U8P, _P]),
    ("stl_shamap_tree_export_device", ctypes.c_int, [_P, _U8P, _U8P, ctypes.c_size_t, _P, _P]),
    ("stl_shamap_nodes_device", ctypes.c_int, [_U8P, _U8P, _P, ctypes.c_size_t, _U8P, _P, _P, _P]),
    ("stl_shamap_nodes", ctypes.c_int, [_U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_tree_apply_nodes_device", ctypes.c_int,
     [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P, _P]),
    ("stl_shamap_tree_apply_nodes", ctypes.c_int, [_P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_tree_lookup_device", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _P, _U8P, _P, _P]),
    ("stl_shamap_tree_lookup", ctypes.c_int, [_P, _U8P, ctypes.c_size_t, _U8P, _U8P, _P]),
    ("stl_shamap_tree_compare_device", ctypes.c_int, [_P, _P, _P, _P]),
    ("stl_shamap_tree_compare", ctypes.c_int, [_P, _P, _P]),
    ("stl_shamap_tree_fork_device", ctypes.c_int, [_P, _P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_tree_fork", ctypes.c_int, [_P, _P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P]),
    ("stl_shamap_tree_fork_nodes_device", ctypes.c_int,
     [_P, _P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P, _P]),
    ("stl_shamap_tree_fork_nodes", ctypes.c_int, [_P, _P, _U8P, _U8P, _U8P, ctypes.c_size_t, _U8P, _P, _P]),
    ("stl_shamap_tree_revert", ctypes.c_int, [_P]),
    ("stl_shamap_tree_fetch_pack_device", ctypes.c_int, [_P, _P, _P, _P, _P]),
    ("stl_shamap_tree_fetch_pack", ctypes.c_int, [_P, _P, _P, _P]),
    ("stl_shamap_tree_get_nodes_device", ctypes.c_int,
     [_P, _P, _P, _P, ctypes.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("stl_shamap_tree_get_nodes", ctypes.c_int, [_P, _P, _P, _P, ctypes.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
]


class ShamapNodesOut(ctypes.Structure):
    """stl_shamap_nodes_out (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_nodes", ctypes.c_uint32), ("hash", ctypes.c_void_p),
                ("body", ctypes.c_void_p), ("id", ctypes.c_void_p), ("meta", ctypes.c_void_p),
                ("count", ctypes.c_void_p)]


class ShamapDiffOut(ctypes.Structure):
    """stl_shamap_diff_out (include/stl.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_rows", ctypes.c_uint32), ("key", ctypes.c_void_p),
                ("kind", ctypes.c_void_p), ("leaf_a", ctypes.c_void_p), ("leaf_b", ctypes.c_void_p),
                ("counts", ctypes.c_void_p)]


VERDICT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)
STL_VERDICT_REJECT, STL_VERDICT_ACCEPT, STL_VERDICT_DEFER = 0, 1, 2


class StlError(RuntimeError):
    def __init__(self, rc, what=""):
        self.rc = rc
        super().__init__(f"libstl error {rc} ({strerror(rc)}) {what}".strip())


_lib = None


def load():
    """Load libstl.so and bind every exported symbol; raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(libstl has no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name, None)
        if fn is None:
            # only an A/B build named by STL_LIB_PATH may predate an entry point
            # (tools/gpujob.sh compares the product with an older build); the
            # product itself exports every one
            if os.environ.get("STL_LIB_PATH"):
                continue
            raise AttributeError(f"{LIB_PATH} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def strerror(rc):
    try:
        return load().stl_strerror(rc).decode()
    except Exception:  # noqa: BLE001 - used while formatting an error
        return "?"


def check(rc, what=""):
    if rc != STL_OK:
        raise StlError(rc, what)
    return rc
