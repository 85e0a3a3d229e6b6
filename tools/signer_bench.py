"""What the signer-authority calls cost, device-resident, in one process:

    a  stl_account_id_batch_device           Hash160 of 2^20 keys
    b  stl_tx_blob_signer_batch_device       the signer pass over the 2^20-blob
                                             ledger of datasets.blob_ledger_plan
    c  stl_signed_blob_verify_batch_device   checkSign of the same blobs

The ledger is built as bench.py's blob leg builds it (signed on the device
over hashlib's signing hashes, 2 % invalid rows).  Its Account fields hold the
synthetic ids of tests/txblob.py, so every STL_TX_OK row is NOT_MASTER; the
kernel's work does not depend on the answer.  Before timing, b's outputs are
checked on a sample of rows against tests/hash160_py.py, and a's against b's
signer IDs.  Then: warm-up, and R rounds of a b c c b a (2 R timed calls per
leg, R >= 10), each call between two device events.  Prints one JSON line
(kept as profiles/signer/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread: a step that overruns ends the process with status 124 before
anything else is started.  The thread runs while the main thread waits inside
the library or in a device synchronise, since ctypes and torch release the
interpreter lock there.  It cannot run while a call holds that lock, nor end a
process the driver will not let go, so on a shared machine also run the tool
under an outer `timeout -k`.

    python3 tools/signer_bench.py [--rounds R] [--step-timeout S] [--out FILE]

Under `rocprofv3 --kernel-trace --stats -- python3 tools/signer_bench.py` the
kernel statistics give tx_signer_kernel beside tx_blob_parse_kernel, the blob
pass it repeats, in the same run.
"""
import argparse
import json
import os
import sys
import threading

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
    from tests import datasets
    from tests.hash160_py import hash160
    dev = torch.device("cuda", 0)
    out = {"tool": "signer_bench", "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
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
    d_pk = torch.from_numpy(np.ascontiguousarray(bp["pks"][bp["who"]])).to(dev)
    ids = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    signer = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    account = torch.empty((n, 20), dtype=torch.uint8, device=dev)
    authority = torch.empty((n,), dtype=torch.uint8, device=dev)
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    status = torch.empty((n,), dtype=torch.uint8, device=dev)
    legs = {
        "a_account_id": lambda: V.account_id_batch_device(d_pk, out=ids, stream=s),
        "b_signer": lambda: V.tx_blob_signer_batch_device(d_buf, d_off, d_len, stream=s, out_signer_id=signer,
                                                         out_account=account, out_authority=authority),
        "c_blob_verify": lambda: V.signed_blob_verify_batch_device(d_buf, d_off, d_len, out_words=words,
                                                                   out_status=status, stream=s),
    }

    def check():
        for fn in legs.values():
            fn()
            fn()  # the verify's automatic dedup follows the previous call's sample
        torch.cuda.synchronize()
        st, au = status.cpu().numpy(), authority.cpu().numpy()
        sg, ac, idh = signer.cpu().numpy(), account.cpu().numpy(), ids.cpu().numpy()
        ok = st == V.TX_OK
        good = bool(np.array_equal(au == V.SIGNER_UNDECIDED, ~ok) and np.array_equal(sg[ok], idh[ok])
                    and not sg[~ok].any())
        rows = np.random.default_rng(1).choice(np.flatnonzero(ok), 200, replace=False)
        for i in rows:
            pk = bp["pks"][bp["who"][i]].tobytes()
            o = int(bp["offs"][i] + bp["p_sig"][i] + 66 + 2)
            acct = bp["buf"][o:o + 20].tobytes()
            good = good and sg[i].tobytes() == hash160(pk) and ac[i].tobytes() == acct
            good = good and au[i] == (V.SIGNER_MASTER if acct == hash160(pk) else V.SIGNER_NOT_MASTER)
        return bool(good), {"ok_rows": int(ok.sum()), "master": int((au == V.SIGNER_MASTER).sum()),
                      "not_master": int((au == V.SIGNER_NOT_MASTER).sum()),
                      "undecided": int((au == V.SIGNER_UNDECIDED).sum()),
                      "accepted": int(V.words_to_bool(words, n).sum())}
    good, counts = step("check", check)
    out["outputs_checked"] = good
    out.update(counts)
    if not good:
        print(json.dumps(out))
        print("the signer pass's outputs are wrong", file=sys.stderr)
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
    med = {k: v["median_ms"] for k, v in out["legs"].items()}
    out["a_keys_per_s"] = round(n / (med["a_account_id"] * 1e-3))
    out["b_rows_per_s"] = round(n / (med["b_signer"] * 1e-3))
    out["b_over_c"] = round(med["b_signer"] / med["c_blob_verify"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
