#!/usr/bin/env python3
"""bench.py -- Ed25519 tx-signature verifies/s on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[1]): 1,048,576 fixed-size Payment-tx
signatures per GPU -- (R||S, 32-byte signing hash, pk) in SoA HBM buffers,
all valid, signed on the GPU from seeded random keys/hashes before timing.
One "step" = one stl_ed25519_verify_batch_device call over the whole batch
(SHA-512(R||A||M), lattice split, decompress A and R, the joint Straus check,
ballot bitmap) plus -- at N > 1 -- libstl's RCCL gather of every rank's accept
bitmap into rank 0 over xGMI (stl_bitmap_gather_device: the path's only
exchange step).  Shards are independent per rank (weak scaling:
every rank verifies its own 1,048,576 signatures, index shard
stl_shard_range(N*n, rank, N)).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--per-gpu N_SIGS] [--dump-outputs DIR] [--full]

A plain run does only what `value` needs: set-up, W warm-up steps, the K timed
steps, the line.  --dump-outputs DIR also writes the last timed step's accept
bitmap as DIR/accepted.npy (float32, one 0/1 value per signature; the inputs
are seeded, so two builds can be compared output for output).  --full adds,
after the timed steps, everything else described below: the per-kernel pass
and its roofline, extra_configs, end_to_end, cpu_baseline.

With N > 1 and no WORLD_SIZE in the environment this process is only a
launcher: it starts `python -m torch.distributed.run --nproc-per-node N ...
bench.py` as a child (one process per GPU) and exits with its code -- it never
touches the GPU itself.  Each rank: torch.distributed over gloo/TCP is the
control plane (barriers, the RCCL unique id, max-over-ranks timing); the data
plane is libstl (verify kernels + RCCL gather).  --dry-run rehearses the
launcher, sharding, control plane and JSON line on CPUs only (no GPU, no
verification; the line says so).

Prints ONE JSON line on rank 0.  roofline: integer-VALU bound; achieved_launch
= W_VERIFY int ops per verify (frozen) x verifies per launch /
average launch time measured with HIP events on the launch stream; with --full
also the main kernel's own figures from libstl's phase clock.
cpu_baseline (--full): the reference's verify call path (libsodium 1.0.18
crypto_sign_verify_detached + stellard S<L, oracle/_ref/libsodium_ref.so) --
or the oracle port when libsodium is absent -- on bounded samples at T = all
affinity CPUs, 16 (the GPU box's CPU share), the cgroup quota, 6 (stellard's
JobQueue default) and 1 threads, median of 5 each, rank 0 at N = 1 only;
`value`/`cores` = the fastest of them, `cpu_quota` = the cgroup's.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Frozen work model (DESIGN.md "Roofline"): 64*N_M + 36*N_S + 5520*B_k with the
# ref10 operation counts N_M = 1520, N_S = 1525 measured by instrumenting the
# oracle's restatement of libsodium's verify (oracle_op_counts), B_k = 1.
W_VERIFY = 64 * 1520 + 36 * 1525 + 5520
# The same work split over the two kernels that do it: phase 1
# (verify_prep_kernel) hashes the one SHA-512 block (5,520) and decompresses A
# and R -- each ge_frombytes_negate_vartime is 19 M + 255 S (oracle op counts,
# tests/test_oracle_golden.py pins them); the second decompression stands in
# for ref10's final inversion (ge_tobytes: 11 M + 254 S), which the half-size
# check never computes.  The main kernel (the Straus loop) gets the rest.
DECODE_OPS = 64 * 19 + 36 * 255
W_PREP = 5520 + 2 * DECODE_OPS
W_MAIN = W_VERIFY - W_PREP
# gfx950 full-rate 32-bit VALU peak: 256 CU x 4 SIMD x 32 lanes x 2.4 GHz
PEAK_INT_OPS = 256 * 4 * 32 * 2.4e9
HBM_PEAK_GBS = 8000.0
BYTES_PER_VERIFY = 64 + 32 + 32 + 1.0 / 8  # algorithmic HBM bytes (sig, msg, pk in; 1 bit out)
# stellard's JobQueue worker count on a big host: min(ncpu, 4) + 2 (JobQueue.cpp:223-236)
JOBQUEUE_THREADS = 6
BOX_CPU_SHARE = 16  # CPUs a one-GPU box grants a job (OMP_NUM_THREADS there)
# deadline of libstl's RCCL bring-up and of the first gathers' wait at N > 1
# (stl_comm_init_rank / stl_comm_sync; one node's bring-up takes seconds)
RCCL_DEADLINE_MS = 60_000


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--per-gpu", dest="n", type=int, default=1 << 20, help="signatures per GPU")
    ap.add_argument("--cpu-threads", type=int, default=BOX_CPU_SHARE)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dry-run", action="store_true", help="launcher/control-plane rehearsal on CPUs, no GPU")
    ap.add_argument("--dry-run-fault", choices=("shift", "dup", "zero"), default=None,
                    help="dry run only: corrupt rank 1's bitmap slice before the gather (the digest check must "
                         "then fail)")
    ap.add_argument("--gather", choices=("rccl", "gloo"), default="rccl",
                    help="bitmap gather at N > 1: libstl's RCCL (the product), or gloo through host memory -- a "
                         "rehearsal of the multi-rank flow with every rank on the visible GPU(s), e.g. 2 ranks on "
                         "a 1-GPU box (RCCL refuses two ranks on one device)")
    ap.add_argument("--no-extra", action="store_true",
                    help="skip the configs[2] / configs[4] / config-1 legs and the end_to_end leg (profiling runs: "
                         "only the bench batch's own launches are traced)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything that is not the headline figure: the per-kernel "
                         "phase-clock pass and the roofline built on it, the extra_configs legs, end_to_end and "
                         "cpu_baseline (--no-extra / --no-cpu-baseline / --cpu-* narrow it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32): accepted = rank 0's "
                         "accept bitmap, one 0/1 value per signature (the gathered bitmap at N > 1)")
    return ap.parse_args()


# --dump-outputs writes at most this many bytes in all
DUMP_CAP_BYTES = 60_000_000


def dump_outputs(dirname, arrays):
    """Each array as DIR/<name>.npy in float32.  An array over its share of
    DUMP_CAP_BYTES is cut to a fixed, seeded sample of its elements (sorted
    indices: the same ones in every run of the same arguments)."""
    os.makedirs(dirname, exist_ok=True)
    cap = (DUMP_CAP_BYTES // len(arrays) - 1024) // 4
    for name, a in arrays.items():
        a = np.asarray(a).reshape(-1)
        if a.size > cap:
            a = a[np.sort(np.random.default_rng(0x5EEDD0).choice(a.size, cap, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), a.astype(np.float32))


# ------------------------------------------------------------------ launcher
def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args):
    """Start one rank per GPU as children (torch.distributed.run) and return
    its exit code.  Nothing here imports torch or touches a device, and the
    process is not replaced (no exec): the ranks are child processes."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    # one node (--nnodes=1): RCCL's bootstrap sockets stay on loopback, so an
    # unresolvable hostname or a down NIC cannot stall ncclCommInitRank
    env.setdefault("NCCL_SOCKET_IFNAME", "lo")
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------ cpu baseline
def affinity_cpus():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)


def cgroup_cpu_quota():
    """CPUs this process's cgroup may use (cgroup v2 cpu.max "quota period",
    v1 cfs_quota_us / cfs_period_us), or None when unlimited / unreadable."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else int(q) / int(per)
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def cpu_baseline(sig, msg, pk, threads_share, reps):
    """Host-core baseline on bounded samples of the same workload, median of
    `reps` runs per thread count: T = the CPUs this process may run on
    (len(sched_getaffinity), SURVEY 8d's "nproc of the GPU box"; the headline
    `value`/`cores`), the box's CPU share (16), 6 (stellard's JobQueue
    default) and 1."""
    from tests import oracle_bind
    lib = oracle_bind.load_sodium_ref()
    if lib is not None:
        kind = "reference"
        what = (f"libsodium {lib.ref_sodium_version().decode()} crypto_sign_verify_detached + S<L "
                "(RippleAddress::verifySignature call path, oracle/_ref/libsodium_ref.so)")

        def run(s, m, p, t):
            return oracle_bind.sodium_verify_batch(lib, s, m, p, threads=t)
    else:
        o = oracle_bind.load_oracle()
        kind = "port"
        what = "oracle/stl_oracle.c restatement"

        def run(s, m, p, t):
            return o.verify_batch(s, m, p, threads=t)
    avail = affinity_cpus()
    quota = cgroup_cpu_quota()
    tquota = max(1, int(round(quota))) if quota else None
    # bounded samples: about 1 s of CPU work per run at each thread count
    # (the whole batch at T = affinity: 16-256 threads on the box)
    plan = [(max(1, avail), 1 << 20), (max(1, threads_share), 1 << 19)]
    if tquota and tquota not in (avail, threads_share):
        plan.append((tquota, 1 << 19))
    plan += [(JOBQUEUE_THREADS, 1 << 18), (1, 1 << 15)]
    rates = {}
    for t, cap in plan:
        if str(t) in rates:
            continue
        n = min(cap, sig.shape[0])
        s, m, p = (np.ascontiguousarray(a[:n]) for a in (sig, msg, pk))
        run(s[:256], m[:256], p[:256], t)  # warm
        times, acc = [], None
        for _ in range(reps):  # noqa: B007
            t0 = time.perf_counter()
            bits = run(s, m, p, t)
            times.append(time.perf_counter() - t0)
            acc = int(bits.sum())
        med = float(np.median(times))
        rates[str(t)] = {"verifies_per_s": n / med, "sample": n, "median_s": med, "runs": reps, "accepted": acc}
    # the headline is the BEST measured thread count: past the
    # box's CPU quota more threads only oversubscribe it
    tbest = max(rates, key=lambda t: rates[t]["verifies_per_s"])
    return {"value": rates[tbest]["verifies_per_s"], "unit": "verifies/s", "cores": int(tbest), "kind": kind,
            "sample": f"first {rates[tbest]['sample']} signatures of the bench batch at T={tbest}, the fastest of "
                      f"T = {', '.join(rates)} (affinity CPUs {avail}, cgroup CPU quota {quota}, box share "
                      f"{threads_share}, stellard's JobQueue default 6, one thread), median of {reps} runs each; "
                      f"{what}",
            "cpu_quota": quota, "by_threads": rates, "host_nproc": os.cpu_count(), "host_affinity_cpus": avail}


def per_kernel(vd, n, kernels):
    """roofline.per_kernel: each kernel's share of the work model over its own
    phase-clock time, with its PMC VALUBusy and instruction-issue bound
    (profiles/valu_latest.json, tools/summarize_valu.py) when present."""
    out = {}
    for name, (work, ms) in kernels.items():
        ach = work * n / (ms * 1e-3) if ms > 0 else 0.0
        k = next((v for kk, v in vd.get("kernels", {}).items() if name in kk), {})
        ib = k.get("issue_bound_ms")
        out[name] = {"work_per_verify": work, "kernel_ms": ms, "achieved": ach / 1e12, "unit": "Tops/s",
                     "frac": ach / PEAK_INT_OPS, "issue_bound_ms": ib,
                     "frac_of_issue_bound": ib / ms if ib and ms > 0 else None,
                     "valu_busy_pct": k.get("VALUBusy"),
                     "valu_insts_per_verify": k["SQ_INSTS_VALU"] * 64 / n if k.get("SQ_INSTS_VALU") else None}
    return out


def end_to_end(V, torch, sig, msgs, pk, reps=5):
    """SURVEY 8d timing (ii): the host batch API on the bench batch --
    stl_ed25519_verify_batch from host buffers: H2D copies, the verify
    kernels, the bitmap D2H (libstl pipelines the copies with the kernels) --
    from pinned (page-locked) and from ordinary pageable memory, median of
    `reps` calls each.  Never `value`."""
    import ctypes
    from stellard_amd import _native as N
    n = sig.shape[0]
    out = {"n": n, "reps": reps}
    B = lambda a: ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ref = None
    for kind in ("pinned", "pageable"):
        if kind == "pinned":
            h = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (sig, msgs, pk)]
            for d, t in zip(h, (sig, msgs, pk)):
                d.copy_(t)
            bm = torch.zeros((n + 7) // 8, dtype=torch.uint8, pin_memory=True)
        else:
            h = [np.ascontiguousarray(t.cpu().numpy()) for t in (sig, msgs, pk)]
            bm = np.zeros((n + 7) // 8, np.uint8)
        lib = N.load()
        call = lambda: N.check(lib.stl_ed25519_verify_batch(B(h[0]), B(h[1]), B(h[2]), n, B(bm), 0),  # noqa: E731
                               "stl_ed25519_verify_batch")
        call()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        bits = np.unpackbits(np.asarray(bm.numpy() if hasattr(bm, "numpy") else bm), bitorder="little")[:n]
        ref = bits if ref is None else ref
        med = float(np.median(ts))
        out[kind] = {"verifies_per_s": n / med, "ms": med * 1e3, "all_accepted": bool(bits.all()),
                     "bits_equal_pinned": bool((bits == ref).all())}
    out["timing"] = ("host steady clock around each stl_ed25519_verify_batch call (H2D of 128 B/signature + "
                     "kernels + D2H of the bitmap, PCIe-inclusive)")
    return out


def config1_leg(V, torch, dev, stream, threads_share):
    """BASELINE configs[0] / SURVEY 8d config 1: 100,000 synthetic Payment
    transactions of 1,000 accounts as whole serialized blobs (Appendix C,
    175-221 B; tests/datasets.py config1_plan: tools/payments.py's rows, 2 %
    of them invalid -- payload / R / S bits flipped after signing, Flags and
    Sequence swapped (DEFERRED), 33-byte keys (MALFORMED)), checkSign from the
    bytes: libstl's device-resident one call stl_signed_blob_verify_batch_device,
    the two-step stl_tx_blob_prepare_device + verify, its host API
    stl_tx_blob_verify_batch (PCIe-inclusive), and the reference's own path on
    the host CPUs -- parse, re-serialise, OpenSSL SHA-512, libsodium verify &&
    S<L (SerializedTransaction.cpp:220-230, Serializer.cpp:354-360,
    RippleAddress.cpp:190-200; oracle/_ref/libsodium_ref.so's
    ref_tx_blob_verify_batch) at T = affinity / box share / 6 / 1.  Bits,
    status bytes and ids are compared with the committed reference digests
    (tests/golden/make_digests.py config1)."""
    import ctypes
    import hashlib
    from tests import datasets, oracle_bind
    from stellard_amd import _native as N
    with open(datasets.DIGESTS) as f:
        want = json.load(f)["config1"]

    def signer_pks(seeds):
        z = torch.zeros((seeds.shape[0], 32), dtype=torch.uint8, device=dev)
        return V.sign_batch_device(torch.from_numpy(np.ascontiguousarray(seeds)).to(dev), z)[0].cpu().numpy()
    plan = datasets.config1_plan(signer_pks)
    n, nacc = plan["n"], datasets.CONFIG1["accounts"]
    msgs = torch.from_numpy(datasets.config1_signing_hashes(plan)).to(dev)
    _, tsig = V.sign_batch_device(torch.from_numpy(np.ascontiguousarray(plan["seeds"][plan["who"]])).to(dev), msgs)
    buf, offs, lens = datasets.config1_finish(plan, tsig.cpu().numpy())
    inputs_ok = datasets.config1_inputs_h16(buf, lens) == want["inputs_h16"]
    d_buf = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_len = torch.from_numpy(lens).to(dev)
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731

    def two_step():
        o = V.tx_blob_prepare_device(d_buf, d_off, d_len, tx_ids=False, stream=stream)
        V.verify_batch_device(o["sig"], o["msg"], o["pk"], out_words=words, stream=stream)
        return o

    def one_call():  # stl_signed_blob_verify_batch_device: the blob pass and verify chunked over two streams
        return V.signed_blob_verify_batch_device(d_buf, d_off, d_len, out_words=words, out_status=status,
                                                 stream=stream)

    def med(fn, reps=21, warm=10):
        # warm calls: the device sat idle while the host legs ran and its clock
        # ramps back over the first ~10 calls of a millisecond each (measured:
        # 1.23 -> 1.11 ms), and the first calls of a stream also settle its
        # automatic-dedup verdict
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    two_s = med(two_step)
    two_bits = V.words_to_bool(words, n)
    dev_s = med(one_call)
    o = V.signed_blob_verify_batch_device(d_buf, d_off, d_len, out_words=words, tx_ids=True, stream=stream)
    torch.cuda.synchronize()
    dev_bits = V.words_to_bool(words, n)
    dev_status = o["status"].cpu().numpy()
    digests = {"inputs_equal": inputs_ok,
               "bitmap_equal": sha(np.packbits(dev_bits, bitorder="little")) == want["bitmap_sha256"],
               "status_equal": sha(dev_status) == want["status_sha256"],
               "ids_equal": sha(o["tx_id"].cpu().numpy()) == want["ids_sha256"],
               "accepted": int(dev_bits.sum()), "accepted_expected": want["accepted"],
               "expected_from": "tests/golden/bitmap_digests.json config1 (make_digests.py: re-serialise + "
                                "OpenSSL + libsodium per row, here in the build container)"}
    B = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bm = np.zeros((n + 7) // 8, np.uint8)
    st = np.zeros(n, np.uint8)
    o64, l32 = offs.astype(np.uint64), lens.astype(np.uint32)
    lib = N.load()
    host = lambda: N.check(lib.stl_tx_blob_verify_batch(B(buf), B(o64), B(l32), n, B(bm), B(st), None, 0),  # noqa: E731
                           "stl_tx_blob_verify_batch")
    host()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        host()
        ts.append(time.perf_counter() - t0)
    host_s = float(np.median(ts))
    host_bits = np.unpackbits(bm, bitorder="little")[:n].astype(bool)
    digests["host_api_bitmap_equal"] = sha(bm) == want["bitmap_sha256"]
    digests["host_api_status_equal"] = sha(st) == want["status_sha256"]
    out = {"n": n, "accounts": nacc, "blob_bytes": {"min": int(lens.min()), "median": int(np.median(lens)),
                                                   "max": int(lens.max())},
           "invalid_rows": int(plan["bad"].size),
           "gpu_device_resident_tx_per_s": n / dev_s, "gpu_device_ms": dev_s * 1e3,
           "gpu_device_two_step_tx_per_s": n / two_s, "two_step_bits_equal": bool((two_bits == dev_bits).all()),
           "gpu_host_api_tx_per_s": n / host_s, "gpu_host_api_ms": host_s * 1e3,
           "status_ok": int((dev_status == V.TX_OK).sum()), "digests": digests,
           "gpu_timing": "host clock around one stl_signed_blob_verify_batch_device call + sync (device-resident; "
                         "two_step: stl_tx_blob_prepare_device + stl_ed25519_verify_batch_device), or around one "
                         "stl_tx_blob_verify_batch call (host API); median"}
    lib_ref = oracle_bind.load_sodium_ref()
    if lib_ref is None:
        out["cpu_reference"] = None
        return out
    blobs = [buf[int(a):int(a) + int(b)].tobytes() for a, b in zip(offs, lens)]
    cpu = {}
    ref_bits = None
    for t, cap in ((affinity_cpus(), n), (threads_share, n), (JOBQUEUE_THREADS, 50_000), (1, 10_000)):
        if str(t) in cpu:
            continue
        m = min(cap, n)
        run = lambda: oracle_bind.sodium_tx_blob_verify_batch(lib_ref, blobs[:m], threads=t)  # noqa: E731
        run()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            bits = run()
            ts.append(time.perf_counter() - t0)
        if m == n and ref_bits is None:
            ref_bits = bits
        cpu[str(t)] = {"tx_per_s": m / float(np.median(ts)), "sample": m, "median_s": float(np.median(ts))}
    out["cpu_reference"] = {"by_threads": cpu, "kind": "reference",
                            "what": "ref_tx_blob_verify_batch: parse + re-serialise (oracle/stl_oracle_tx.c) + "
                                    "OpenSSL SHA512 + libsodium 1.0.18 crypto_sign_verify_detached && S<L, "
                                    "std::thread-style static partition, median of 3"}
    if ref_bits is not None:
        # the device contract: the reference's bit where the row's status is
        # OK; deferred rows (the reference accepts them) go to the caller
        ok = dev_status == V.TX_OK
        out["bitmap_parity"] = {"rows": n, "reference_accepted": int(ref_bits.sum()),
                                "mismatches_device": int((dev_bits != (ref_bits & ok)).sum()),
                                "mismatches_host_api": int((host_bits != (ref_bits & ok)).sum()),
                                "deferred_rows_reference_accepts": int((ref_bits & (dev_status == V.TX_DEFERRED)).sum())}
    return out


# ------------------------------------------------------------------ ranks
def control_plane(world, rank):
    import torch.distributed as dist
    if world > 1:
        # one node: gloo's and RCCL's bootstrap sockets on loopback, whoever
        # launched the ranks (this launcher or the driver's torch.distributed.run)
        # -- a hostname that does not resolve cannot stall the rendezvous
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        dist.init_process_group("gloo")
    return dist


def dry_run(args, world, rank):
    """CPU rehearsal: launcher, shard ranges, gloo control plane, the gather
    of bitmap words over gloo, max-over-ranks timing and the JSON line.  No
    GPU, no verification: ``value`` counts gathered bitmap words only."""
    import torch
    dist = control_plane(world, rank)
    from stellard_amd import shard
    n = args.n
    lo, hi = shard.shard_range(n * world, rank, world)
    words = torch.full((shard.words_per_rank(n * world, world),), -1, dtype=torch.int64)
    for _ in range(args.warmup):
        full = shard.gather_bitmap_words(words, n * world, world, dist) if world > 1 else words
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        full = shard.gather_bitmap_words(words, n * world, world, dist) if world > 1 else words
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t[0])
    ok = bool(shard.words_to_bool(full, n * world).all())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"accepted": shard.words_to_bool(full, n * world)})
    from tools import bench_legs as BL
    ctx = {"world": world, "rank": rank, "dist": dist, "sync": lambda: None,
           "gather": BL.Gather(world, rank, dist, "gloo")}
    rehearsal = BL.dry_digest_leg(ctx, fault=args.dry_run_fault)
    if rank == 0:
        print(json.dumps({
            "metric": "DRY RUN (launcher rehearsal, no GPU, no verification)", "value": n * world * args.steps / dt,
            "unit": "bitmap bits gathered/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt * 1e3 / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32", "data": "synthetic", "dry_run": True,
            "config": {"workload": "dry run", "signatures_per_gpu": n, "parallelism": f"dp{world}",
                       "rank0_shard": [lo, hi], "gathered_all_ones": ok,
                       "rccl_nranks": world, "rccl_nranks_source": "stub (dry run: no RCCL communicator; the GPU "
                                                                   "run reads libstl's stl_comm_info)"},
            "roofline": None, "cpu_baseline": None,
            "extra_configs": {"digest_rehearsal": rehearsal}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def extra_configs(ctx):
    """The other configs of BASELINE.json, measured after the timed bench steps
    at every N and reported under ``extra_configs`` (not ``value``), each
    proving bit-exactness of the gathered bitmap against libsodium's digest
    (tools/bench_legs.py): configs[2] (64M, adversarial, block shards,
    ncclGather), configs[3] (10M adversarial, unequal block shards, grouped
    send/recv) and configs[4] (one ledger split by preimage bytes).  A leg
    whose inputs fail on any rank reports the error on every rank before any
    collective of that leg runs."""
    from tools import bench_legs as BL
    out = {}
    for key, fn in (("config3_64M_digest", lambda: BL.digest_leg(ctx, "config3")),
                    ("config4_10M_digest", lambda: BL.digest_leg(ctx, "config4")),
                    ("config5_ledger_split", lambda: BL.ledger_leg(ctx)),
                    ("config5_blob_split", lambda: BL.blob_ledger_leg(ctx))):
        try:
            out[key] = fn()
        except Exception as e:  # noqa: BLE001 - reported, never fatal to the bench line
            out[key] = {"error": f"rank {ctx['rank']}: {e!r}"}
        ctx["sync"]()
    return out


def gpu_run(args, world, rank, local):
    import torch
    dist = control_plane(world, rank)
    rehearsal = world > 1 and args.gather == "gloo"
    torch.cuda.set_device(local % torch.cuda.device_count() if rehearsal else local)
    from stellard_amd import verify as V

    V.init(device_count=1, first_device=torch.cuda.current_device())
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.n
    lo, hi = V.shard_range(n * world, rank, world)
    assert (lo, hi) == (rank * n, (rank + 1) * n) or n % 64, "per-rank shards are whole ballot words"
    gather_via = None
    rccl_nranks = None
    if rehearsal:
        gather_via = "gloo through host memory (rehearsal of the multi-rank flow, not the RCCL product path)"
    elif world > 1:
        # rank 0 makes the RCCL unique id; gloo carries it to every rank.  The
        # bring-up runs under libstl's RCCL deadline (RCCL_DEADLINE_MS: a rank
        # that never joins is STL_ERCCL, not a hang -- VERDICT r4 #3); if
        # libstl's communicator cannot be built on some rank, every rank falls
        # back to the gloo gather through host memory and the line says so.
        V.debug_tuning(V.TUNE_RCCL_TIMEOUT_MS, RCCL_DEADLINE_MS)
        obj = [None]
        if rank == 0:
            try:
                obj = [V.comm_unique_id()]
            except Exception as e:  # noqa: BLE001
                obj = [f"ERR {e!r}"]
        dist.broadcast_object_list(obj, src=0)
        err = obj[0] if isinstance(obj[0], str) else None
        if err is None:
            try:
                V.comm_init_rank(world, rank, obj[0])
            except Exception as e:  # noqa: BLE001
                err = repr(e)
        errs = [None] * world
        dist.all_gather_object(errs, err)
        if any(errs):
            if err is None:
                V.comm_abort()
            rehearsal = True  # gloo through host memory from here on
            gather_via = ("gloo through host memory (libstl RCCL communicator failed on some rank: %s)"
                          % next(e for e in errs if e))
        else:
            gather_via = "libstl stl_bitmap_gather_device (ncclGather to rank 0)"
            # what RCCL itself says the communicator is (ncclCommCount /
            # ncclCommUserRank): every rank must see all N ranks before timing
            rccl_nranks, rccl_rank = V.comm_info()
            if rccl_nranks != world or rccl_rank != rank:
                raise SystemExit(f"rank {rank}: RCCL communicator reports rank {rccl_rank} of {rccl_nranks}, "
                                 f"WORLD_SIZE={world}")

    # ---- synthetic data (outside the timed region) ----
    rng = np.random.default_rng(0x5EED0002 + rank)
    seeds = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    msgs = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    pk, sig = V.sign_batch_device(seeds, msgs)
    torch.cuda.synchronize()
    wpr = (n + 63) // 64
    words = torch.empty(wpr, dtype=torch.int64, device=dev)
    full_words = torch.empty(wpr * world, dtype=torch.int64, device=dev) if world > 1 and rank == 0 else None
    stream = torch.cuda.current_stream()

    from tools.bench_legs import Gather, words_h16
    gather_into = Gather(world, rank, dist, "gloo" if rehearsal else "rccl", V=V, stream=stream)
    woffs = np.arange(world + 1, dtype=np.uint64) * wpr
    if rehearsal and rank == 0:
        full_words = full_words.cpu()

    def gather():
        gather_into(words, woffs, full_words)

    def step():
        V.verify_batch_device(sig, msgs, pk, out_words=words, stream=stream)
        if world > 1:
            gather()

    for _ in range(args.warmup):
        step()
    if world > 1 and gather_into.mode == "rccl":
        # the first RCCL gathers, waited for under the deadline: a peer that
        # never posts its slice aborts the communicator instead of hanging
        # this rank; then every rank switches to the gloo gather together
        err = None
        try:
            V.comm_sync(stream, RCCL_DEADLINE_MS)
        except Exception as e:  # noqa: BLE001
            err = repr(e)
        errs = [None] * world
        dist.all_gather_object(errs, err)
        if any(errs):
            V.comm_abort()
            gather_into.mode = "gloo"
            if rank == 0:
                full_words = full_words.cpu()
            gather_via = ("gloo through host memory (libstl RCCL gather did not complete within %d ms on some "
                          "rank: %s)" % (RCCL_DEADLINE_MS, next(e for e in errs if e)))
            for _ in range(args.warmup):
                step()
    torch.cuda.synchronize()
    ok = V.words_to_bool(words, n)
    if not ok.all():
        raise SystemExit(f"rank {rank}: {int((~ok).sum())} valid signatures rejected -- parity failure")

    # ---- timed region: exactly K steps between barrier+sync on both sides ----
    # shader-clock stamps (stl_debug_clock_stamp) right before and right after
    # it, both outside it: the chip's average clock over the timed launches
    # (boxes hold 2.1-2.3 GHz under this load)
    clk0 = V.clock_stamp(256, stream)
    torch.cuda.synchronize()
    V.set_phase_timing(False)
    V.reset_stats()
    if world > 1:
        dist.barrier()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        ev[k][0].record(stream)
        V.verify_batch_device(sig, msgs, pk, out_words=words, stream=stream)
        ev[k][1].record(stream)
        if world > 1:
            gather()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    clk1 = V.clock_stamp(256, stream)
    torch.cuda.synchronize()
    clock_ghz, clock_xcc, clock_cus = V.clock_ghz(clk0, clk1)
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    t = torch.tensor([dt, kern_ms], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt, kern_ms = float(t[0]), float(t[1])
    gathered_check = None
    if world > 1:
        # every rank's slice must sit at its own offset of the gathered buffer:
        # rank 0 compares each slice with that rank's own words (digests over
        # gloo), so a misplaced, duplicated or stale slice fails the line
        own = [None] * world
        dist.all_gather_object(own, words_h16(words))
        if rank == 0:
            at = [words_h16(full_words[r * wpr:(r + 1) * wpr]) for r in range(world)]
            gathered_check = {"slices_equal_rank_words": at == own,
                              "all_accepted": bool(V.words_to_bool(full_words, n * world).all())}
            assert gathered_check["slices_equal_rank_words"], "gathered bitmap slices differ from the ranks' words"
            assert gathered_check["all_accepted"], "gathered bitmap has rejects"

    st = V.get_stats()  # device counters over the K timed launches (after the sync above)
    if rank == 0 and args.dump_outputs:
        # what the caller of the last timed step holds: the accept bitmap
        # (gathered from every rank at N > 1), before any later leg reuses the buffers
        dump_outputs(args.dump_outputs, {"accepted": V.words_to_bool(full_words if world > 1 else words, n * world)})
    if rank == 0:
        line = headline(args, world, n, dt, kern_ms, (clock_ghz, clock_xcc, clock_cus), V.execution_settings(),
                        {"gather": gather_via, "rccl_nranks": rccl_nranks, "gather_check": gathered_check}, st)
    if args.full:
        full_report(args, world, rank, line if rank == 0 else None, kern_ms,
                    {"dist": dist, "V": V, "torch": torch, "dev": dev, "stream": stream, "gather": gather_into},
                    (sig, msgs, pk, words))
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        if gather_into.mode == "rccl":
            V.comm_destroy()
        dist.destroy_process_group()


def headline(args, world, n, dt, kern_ms, clock, execution, gather, st):
    """Rank 0's result line of a plain run: the timed steps' figures only.
    roofline holds what the timed launches' own HIP events give; the
    per-kernel figures take launches of their own (--full, full_report)."""
    clock_ghz, clock_xcc, clock_cus = clock
    per_launch = n / (kern_ms * 1e-3)
    achieved_launch = W_VERIFY * per_launch / 1e12
    return {
        "metric": "Ed25519 tx verifies/sec",
        "value": n * world * args.steps / dt,
        "unit": "verifies/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt * 1e3 / args.steps,
        "clock_ghz": clock_ghz,
        "cycles_per_verify": (dt / args.steps) * clock_ghz * 1e9 / n if clock_ghz else None,
        "clock": {"per_xcc_ghz": clock_xcc, "cus_matched": clock_cus,
                  "how": "stl_debug_clock_stamp (one wave per workgroup, 256 workgroups) right before and "
                         "right after the timed region: per CU, d(s_memtime) / d(s_memrealtime) x 100 MHz, "
                         "median over the CUs stamped both times (rank 0's GPU); cycles_per_verify = "
                         "ms_per_step x clock_ghz / signatures per GPU"},
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic: GPU-signed RFC 8032 signatures over seeded random keys and 32-byte signing hashes",
        "full": bool(args.full),
        "config": {"workload": "configs[1]: 1,048,576 fixed-size Payment-tx signatures per GPU "
                               "(stl_ed25519_verify_batch_device, policy libsodium-1.0.18 + S<L)",
                   "signatures_per_gpu": n,
                   "parallelism": f"dp{world} (index shards, RCCL bitmap gather to rank 0)"
                                  if world > 1 else "dp1",
                   "gather": gather["gather"], "rccl_nranks": gather["rccl_nranks"],
                   "gather_check": gather["gather_check"],
                   "execution": dict(execution,
                                     stream_pool="libstl: 2 kernel + 1 copy streams per device, made in "
                                                 "stl_init before any caller stream (DESIGN.md section 8); "
                                                 "chunk_log2 0 = round(n / 2^18) equal chunks")},
        "roofline": {"bound": "valu", "peak": PEAK_INT_OPS / 1e12, "unit": "Tops/s",
                     "algorithmic_bytes": BYTES_PER_VERIFY * n,
                     "work_model": "W_VERIFY = 64*1520 M + 36*1525 S + 5520 (ref10 verify) = %d ops; main "
                                   "kernel W_MAIN = W_VERIFY - W_PREP = %d, prep W_PREP = SHA-512 block + two "
                                   "decompressions = %d" % (W_VERIFY, W_MAIN, W_PREP),
                     "launch_ms": kern_ms, "achieved_launch": achieved_launch,
                     "frac_launch": achieved_launch * 1e12 / PEAK_INT_OPS,
                     "launch": "every kernel of one stl_ed25519_verify_batch_device call (phase 1, main, "
                               "fallback), HIP events around each call of the timed region",
                     "hbm_frac": BYTES_PER_VERIFY * per_launch / (HBM_PEAK_GBS * 1e9)},
        "cpu_baseline": None,
        "stats": {"source": "stl_get_stats over the timed launches (rank 0)",
                  "accepted": st["accepted"], "full_length_lanes": st["full_length_lanes"],
                  "verifies": n * args.steps},
        "extra_configs": None,
    }


def full_report(args, world, rank, line, kern_ms, ctx, batch):
    """--full: everything past the headline figure, run after the timed
    region on every rank (the legs gather); rank 0 adds the results to
    ``line`` (None on the other ranks)."""
    V, torch, stream = ctx["V"], ctx["torch"], ctx["stream"]
    sig, msgs, pk, words = batch
    n = args.n
    # ---- per-kernel timing pass: K more launches with libstl's phase clock --
    # HIP events recorded on the launch stream between the kernels of each
    # launch, which runs its kernels one after another (no concurrent chunks),
    # so each duration is that kernel's alone ----
    V.set_phase_timing(True)
    V.reset_stats()
    for _ in range(args.steps):
        V.verify_batch_device(sig, msgs, pk, out_words=words, stream=stream)
    torch.cuda.synchronize()
    pst = V.get_stats()
    V.set_phase_timing(False)
    extra = None
    if not args.no_extra:
        extra = extra_configs(dict(ctx, world=world, rank=rank, sync=torch.cuda.synchronize))
    chunks = max(1, pst["phase_chunks"])
    phase_ms = {k: v / chunks / 1e6 for k, v in pst["phase_ns"].items()}  # average per launch (one chunk each)
    if rank == 0:
        # the dominant kernel (verify_main_kernel): algorithmic work of one
        # launch (W_VERIFY x n) / its average duration, live HIP events
        main_ms = phase_ms["main"]
        prep_ms = phase_ms["phase1"]
        achieved = W_MAIN * n / (main_ms * 1e-3) / 1e12
        traffic, traffic_build = None, None
        from stellard_amd.build import source_digest
        digest = source_digest()

        def provenance(doc, path):
            b = dict(doc.get("build") or {})
            b["file"] = os.path.relpath(path, ROOT)
            b["matches_current_sources"] = b.get("sources_sha256") == digest
            return b
        tp = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tp):
            with open(tp) as f:
                td = json.load(f)
            traffic = (td.get("main_kernel") or {}).get("hbm_bytes_per_launch")
            traffic_build = provenance(td, tp)
        valu_busy, issue, vd = None, None, {}
        vp = os.path.join(ROOT, "profiles", "valu_latest.json")
        if os.path.exists(vp):
            with open(vp) as f:
                vd = json.load(f)
            mk = next((v for k, v in vd.get("kernels", {}).items() if "verify_main_kernel" in k), {})
            if mk.get("issue_bound_ms"):
                issue = {"issue_bound_ms": mk["issue_bound_ms"], "frac_of_issue_bound": mk["issue_bound_ms"] / main_ms,
                         "effective_clock_ghz": mk.get("effective_clock_ghz"),
                         "model": mk.get("issue_bound_model"),
                         "source": "profiles/valu_latest.json (main kernel PMC instruction counts)"}
            valu_busy = {"launch_pct": vd.get("launch_valu_busy_pct"),
                         "per_kernel_pct": {k: v.get("VALUBusy") for k, v in vd.get("kernels", {}).items()},
                         "source": vd.get("source", "rocprofv3 --pmc VALUBusy, profiles/valu_latest.json"),
                         "build": provenance(vd, vp)}
        line["config"]["execution"]["overlap"] = {
            "serial_kernel_sum_ms": sum(phase_ms.values()), "launch_ms": kern_ms,
            "ratio": kern_ms / max(1e-9, sum(phase_ms.values())),
            "reading": "ratio < 1: the chunks on the pool's two kernel streams overlapped; >= 1: they ran one "
                       "after another (e.g. streams sharing a hardware queue)"}
        line["roofline"].update({
            "achieved": achieved, "frac": achieved * 1e12 / PEAK_INT_OPS, "traffic": traffic,
            "per_kernel": per_kernel(vd, n, {"verify_prep_kernel": (W_PREP, prep_ms),
                                             "verify_main_kernel": (W_MAIN, main_ms)}),
            "traffic_over_algorithmic": traffic / (BYTES_PER_VERIFY * n) if traffic else None,
            "traffic_build": traffic_build, "sources_sha256": digest,
            "kernel": "verify_main_kernel (dominant: %.0f %% of the launch)"
                      % (100.0 * main_ms / max(1e-9, sum(phase_ms.values()))),
            "kernel_ms": main_ms, "work_per_verify": W_MAIN, "units_per_launch": n,
            "timing": "libstl phase events (stl_set_phase_timing) on the launch stream over K "
                      "launches right after the timed region (kernels one after another); work = "
                      "W_MAIN x n per launch, the part of W_VERIFY the main kernel does",
            "frac_all_work_on_main": W_VERIFY * n / (main_ms * 1e-3) / PEAK_INT_OPS,
            "phase_ms": phase_ms,
            "valu_busy_pmc": valu_busy,
            "issue_bound": issue})
        line["extra_configs"] = extra
        if world == 1 and not args.no_extra:
            try:
                line["end_to_end"] = end_to_end(V, torch, sig, msgs, pk)
            except Exception as e:  # noqa: BLE001 - reported, never fatal to the bench line
                line["end_to_end"] = {"error": repr(e)}
        if world == 1 and not args.no_extra:
            try:
                c1 = config1_leg(V, torch, ctx["dev"], stream, args.cpu_threads)
            except Exception as e:  # noqa: BLE001
                c1 = {"error": repr(e)}
            line["extra_configs"] = dict(line["extra_configs"] or {}, config1_payment_checksign_100k=c1)
        if world == 1 and not args.no_cpu_baseline:
            try:
                line["cpu_baseline"] = cpu_baseline(sig.cpu().numpy(), msgs.cpu().numpy(), pk.cpu().numpy(),
                                                    args.cpu_threads, args.cpu_reps)
            except Exception as e:  # noqa: BLE001 - the baseline must not kill the GPU number
                line["cpu_baseline"] = {"error": repr(e)}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}: one rank per GPU")
    if args.dry_run:
        dry_run(args, world, rank)
    else:
        gpu_run(args, world, rank, local)


if __name__ == "__main__":
    main()
