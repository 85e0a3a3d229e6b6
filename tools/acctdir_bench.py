"""What the account directory costs, in one process:

    a  stl_tx_blob_signer_batch_device        today's call: the baseline
    b  stl_acctdir_tx_blob_authority_device   checkSig's verdict per row
    c  stl_acctdir_lookup_device              the bare map, 2^20 IDs
    d  stl_acctdir_upsert                     2^20 fresh accounts into an empty
                                              directory, and 4,096 fresh ones
                                              into the loaded one (host-inclusive
                                              wall times)

over the 2^20-blob ledger of datasets.blob_ledger_plan, built as
tools/signer_bench.py builds it, with the distinct Account values of that
ledger upserted first (flags by account number mod 4; of every fourth account
the RegularKey is the signer of its first row, so REGULAR occurs).  Before
timing, b's verdicts are checked on a sample of rows against
tests/acctdir_py.check_sig, its IDs against a's bit for bit, and c's answers
against the entries.  Then: warm-up, and R rounds of a b c c b a (2 R timed
calls per leg, R >= 10), each call between two device events.  Prints one JSON
line (kept as profiles/acctdir/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread as in tools/signer_bench.py; on a shared machine also run the
tool under an outer `timeout -k`.

    python3 tools/acctdir_bench.py [--rounds R] [--step-timeout S] [--out FILE]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
            "max_ms": round(float(a.max()), 4), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("--rounds >= 10 (20 timed calls per leg)")
    import torch
    from stellard_amd import build, verify as V
    from tests import acctdir_py as AP
    from tests import datasets
    dev = torch.device("cuda", 0)
    out = {"tool": "acctdir_bench", "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "source_digest": build.source_digest()[:16]}

    def step(name, fn):
        def overrun():
            print(f"step {name!r} overran {args.step_timeout} s", file=sys.stderr, flush=True)
            os._exit(124)
        dog = threading.Timer(args.step_timeout, overrun)
        dog.daemon = True
        dog.start()
        try:
            r = fn()
            torch.cuda.synchronize()
            return r
        finally:
            dog.cancel()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step("init", V.init)
    s = torch.cuda.current_stream()

    def ledger():
        def signer_pks(seeds):
            z = torch.zeros((seeds.shape[0], 32), dtype=torch.uint8, device=dev)
            return V.sign_batch_device(torch.from_numpy(np.ascontiguousarray(seeds)).to(dev), z)[0].cpu().numpy()
        bp = datasets.blob_ledger_plan(signer_pks)
        msgs = torch.from_numpy(datasets.blob_signing_hashes(bp)).to(dev)
        _, sig = V.sign_batch_device(torch.from_numpy(np.ascontiguousarray(bp["seeds"][bp["who"]])).to(dev), msgs)
        datasets.blob_ledger_finish(bp, sig.cpu().numpy())
        return bp
    bp = step("ledger", ledger)
    n = bp["n"]
    out["rows"] = n
    out["blob_bytes"] = int(bp["total"])
    d_buf = torch.from_numpy(bp["buf"]).to(dev)
    d_off = torch.from_numpy(bp["offs"]).to(dev)
    d_len = torch.from_numpy(bp["lens"]).to(dev)
    signer = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    account = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    master = torch.empty((n,), dtype=torch.uint8, device=dev)
    signer_b = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    account_b = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    authority = torch.empty((n,), dtype=torch.uint8, device=dev)
    flags_c = torch.empty((n,), dtype=torch.uint8, device=dev)
    keys_c = torch.empty((n, 20), dtype=torch.uint8, device=dev)

    def a_signer():
        return V.tx_blob_signer_batch_device(d_buf, d_off, d_len, stream=s, out_signer_id=signer, out_account=account,
                                             out_authority=master)

    # the ledger's accounts, from today's call
    def entries():
        a_signer()
        torch.cuda.synchronize()
        decided = np.flatnonzero(master.cpu().numpy() != V.SIGNER_UNDECIDED)
        acct, first = np.unique(account.cpu().numpy()[decided], axis=0, return_index=True)
        m = acct.shape[0]
        flags = (np.arange(m) % 4).astype(np.uint8)
        keys = np.random.default_rng(2).integers(0, 256, (m, 20), dtype=np.uint8)
        every4 = np.arange(m) % 4 == 1
        keys[every4] = signer.cpu().numpy()[decided[first[every4]]]
        return np.ascontiguousarray(acct), flags, keys
    acct, flags, keys = step("entries", entries)
    m = acct.shape[0]
    out["accounts"] = m
    rng = np.random.default_rng(3)

    def fresh(count):
        return rng.integers(0, 256, (count, 20), dtype=np.uint8), rng.integers(0, 4, count).astype(np.uint8), \
            rng.integers(0, 256, (count, 20), dtype=np.uint8)

    small_reps = 10
    directory = V.AccountDirectory(m + 4096 * (small_reps + 2))
    step("upsert", lambda: directory.upsert(acct, flags, keys))
    out["directory"] = directory.info()

    legs = {
        "a_signer": a_signer,
        "b_authority": lambda: directory.tx_blob_authority_device(
            d_buf, d_off, d_len, stream=s, out_signer_id=signer_b, out_account=account_b, out_authority=authority),
        "c_lookup": lambda: directory.lookup_device(account, stream=s, out_flags=flags_c, out_regular_key=keys_c),
    }

    def check():
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        au, ms = authority.cpu().numpy(), master.cpu().numpy()
        sg, ac = signer.cpu().numpy(), account.cpu().numpy()
        good = bool(np.array_equal(sg, signer_b.cpu().numpy()) and np.array_equal(ac, account_b.cpu().numpy()))
        good = good and bool(np.array_equal(au == V.AUTH_UNDECIDED, ms == V.SIGNER_UNDECIDED))
        state = {acct[i].tobytes(): (int(flags[i]), keys[i].tobytes()) for i in range(m)}
        fl, ky = flags_c.cpu().numpy(), keys_c.cpu().numpy()
        rows = np.random.default_rng(1).choice(np.flatnonzero(ms != V.SIGNER_UNDECIDED), 2000, replace=False)
        for i in rows:
            f, k = state[ac[i].tobytes()]
            entry = AP.Entry(k if f & AP.HAS_REGULAR_KEY else None, bool(f & AP.MASTER_DISABLED))
            good = good and au[i] == AP.check_sig(sg[i].tobytes(), ac[i].tobytes(), entry)
            good = good and fl[i] == f and ky[i].tobytes() == (k if f & AP.HAS_REGULAR_KEY else bytes(20))
        und = ms == V.SIGNER_UNDECIDED  # zero accounts: not in the directory
        good = good and bool((fl[und] == V.ACCT_NOT_FOUND).all())
        return bool(good), {"verdicts": [int(x) for x in np.bincount(au, minlength=7)]}
    good, counts = step("check", check)
    out["outputs_checked"] = good
    out.update(counts)
    if not good:
        print(json.dumps(out))
        print("the directory's outputs are wrong", file=sys.stderr)
        sys.exit(1)

    def ab():
        ts = {k: [] for k in legs}
        for k in legs:  # warm-up
            legs[k]()
            legs[k]()
        torch.cuda.synchronize()
        order = list(legs) + list(legs)[::-1]
        for _ in range(args.rounds):
            for k in order:
                ts[k].append(timed(legs[k]))
        return ts
    ts = step("ab", ab)
    out["legs"] = {k: spread(v) for k, v in ts.items()}

    # d: upserts, host-inclusive wall time
    def upsert_small():
        ms = []
        for _ in range(small_reps + 1):  # the first grows the staging buffer: not counted
            batch = fresh(4096)
            t0 = time.perf_counter()
            directory.upsert(*batch)
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms[1:]
    out["legs"]["d_upsert_4096_loaded"] = spread(step("upsert_small", upsert_small))
    directory.close()

    # ... and, while a directory of 2^20 accounts exists, the bare map on it: 2^20 of its IDs in
    # random order (the ledger's own directory is small enough to stay in cache)
    big_lookup = []

    def upsert_big():
        ms = []
        for _ in range(3):
            batch = fresh(1 << 20)
            with V.AccountDirectory(1 << 20) as d:
                t0 = time.perf_counter()
                d.upsert(*batch)
                ms.append((time.perf_counter() - t0) * 1e3)
                out["big_directory"] = d.info()
                q = torch.from_numpy(batch[0][rng.permutation(1 << 20)]).to(dev)
                look = lambda: d.lookup_device(q, stream=s, out_flags=flags_c, out_regular_key=keys_c)  # noqa: E731
                look()
                big_lookup.extend(timed(look) for _ in range(7))
                found = flags_c.cpu().numpy() != V.ACCT_NOT_FOUND
                out["big_directory_found"] = int(found.sum())
        return ms
    out["legs"]["d_upsert_2e20_empty"] = spread(step("upsert_big", upsert_big))
    out["legs"]["c_lookup_2e20_accounts"] = spread(big_lookup)

    med = {k: v["median_ms"] for k, v in out["legs"].items()}
    out["b_over_a"] = round(med["b_authority"] / med["a_signer"], 4)
    out["b_rows_per_s"] = round(n / (med["b_authority"] * 1e-3))
    out["c_ids_per_s"] = round(n / (med["c_lookup"] * 1e-3))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
