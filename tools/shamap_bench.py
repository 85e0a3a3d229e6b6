"""What the SHAMap root (stl_shamap_root_device) costs, device-resident, on one GPU:

    random_2^20      2^20 uniformly random IDs
    random_2^16      2^16 uniformly random IDs
    clustered_2^20   2^20 IDs in 4,096 clusters that share 40 nibbles
    ledger_2^20      the IDs stl_signed_blob_verify_batch_device writes for the
                     2^20-blob ledger of datasets.blob_ledger_plan, with that
                     call's accept words as the select bitmap; and, in the same
                     run, that verify call itself: the root as a share of the
                     check it follows

For each input the whole call, 20 calls each between two device events (median,
min, max).  Then, in calls of their own with stl_set_phase_timing on, the
library's own marks: sort (the four radix passes and, with a select bitmap, the
one-bit pass), prepare (heads, scan, compaction, neighbour bytes), levels (the
64 level launches) and finish, each over 20 calls as well.  Before timing, the
counts of every input are checked for consistency, and the 2^16 root against
the Python model (tests/shamap_py.py).  Prints one JSON line (kept as
profiles/shamap/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_bench.py [--calls C] [--no-ledger] [--step-timeout S] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-ledger", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from stellard_amd import build, verify as V
    from tests import datasets, shamap_py as SM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "source_digest": build.source_digest()[:16], "inputs": {}}

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
    root = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)

    def measure(name, keys, words=None, extra=None):
        """keys: (n, 32) uint8 on the device."""
        n = keys.shape[0]

        def call():
            V.shamap_root_device(keys, None, words, out_root=root, counts=cnt, stream=s)

        def legs():
            call()
            call()  # the workspace has its size
            torch.cuda.synchronize()
            c = [int(x) for x in cnt.cpu().numpy()]
            whole = [timed(call) for _ in range(args.calls)]
            was = V.set_phase_timing(True)
            phases = []
            try:
                for _ in range(args.calls):
                    torch.cuda.synchronize()
                    V.reset_stats()
                    call()
                    torch.cuda.synchronize()
                    st = V.get_stats()
                    if st["phase_chunks"] == 1:
                        phases.append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
            finally:
                V.set_phase_timing(was)
            return c, whole, phases
        c, whole, phases = step(name, legs)
        rec = {"rows": int(n), "select_bitmap": words is not None, "counts": c, "root": root.cpu().numpy().tobytes().hex(),
               "whole_call": spread(whole)}
        if phases:
            for i, ph in enumerate(("sort", "prepare", "levels", "finish")):
                rec[ph] = spread([p[i] for p in phases])
        if extra:
            rec.update(extra)
        out["inputs"][name] = rec
        return rec

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # the model's word on the smallest input
    k16 = SM.case_keys("random65536", 16)
    r16 = measure("random_2^16", on_device(k16))
    want = SM.model(k16)
    out["model_checked"] = (r16["root"], r16["counts"]) == (want[0].hex(), want[1])
    if not out["model_checked"]:
        print(json.dumps(out))
        print("the 2^16 root differs from the model's", file=sys.stderr)
        sys.exit(1)
    r = measure("random_2^20", on_device(SM.case_keys("random1048576", 20)))
    assert r["counts"][0] + r["counts"][1] == 1 << 20
    r = measure("clustered_2^20", on_device(SM.case_keys("cluster1048576_4096_40", 21)))
    assert r["counts"][0] + r["counts"][1] == 1 << 20 and r["counts"][3] >= 40

    if not args.no_ledger:
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
        d_buf, d_off, d_len = on_device(bp["buf"]), on_device(bp["offs"]), on_device(bp["lens"])
        words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        ids = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

        def verify():
            V.signed_blob_verify_batch_device(d_buf, d_off, d_len, out_words=words, out_status=status, out_ids=ids,
                                              stream=s)

        def verify_legs():
            verify()
            verify()
            torch.cuda.synchronize()
            return [timed(verify) for _ in range(args.calls)]
        vt = step("verify", verify_legs)
        accepted = int(V.words_to_bool(words, n).sum())
        r = measure("ledger_2^20", ids, words, {"blob_bytes": int(bp["total"]), "accepted_rows": accepted,
                                                 "signed_blob_verify": spread(vt)})
        assert r["counts"][0] + r["counts"][1] == accepted
        r["root_over_verify"] = round(r["whole_call"]["median_ms"] / r["signed_blob_verify"]["median_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
