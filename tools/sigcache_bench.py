"""What the verified-ID cache costs and saves, in one process:

    a  stl_signed_blob_verify_batch_device            today's call: the yardstick
    b  stl_sigcache_signed_blob_verify_batch_device   cold: stl_sigcache_clear (and a
                                                      synchronize) before each timed call
    c  the same, warm: every row seen before
    d  the same, half the rows seen before (cleared, then the first half verified,
       before each timed call)
    e  stl_sigcache_lookup_device                     the bare probe of the 2^20 IDs

over the 2^20-blob ledger of datasets.blob_ledger_plan, device-resident, built
as tools/acctdir_bench.py builds it.  Before timing, the cached call's bits,
status and IDs are checked against a's, cold and warm.  Then 20 timed calls per
leg, in rounds of a b c d e e d c b a, each call between two device events (the
cached call's one host wait lies between them); min, median and max per leg,
the hits and verified counts of each leg, and each leg's ratio to a.  Prints
one JSON line (kept as profiles/sigcache/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/sigcache_bench.py [--rounds R] [--sets-log2 K] [--only LEG] [--step-timeout S] [--out FILE]

--only LEG (a .. e) runs the warm-up and that leg alone, 20 calls: the run to
put under a kernel trace.
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
    ap.add_argument("--sets-log2", type=int, default=22)
    ap.add_argument("--only", default="", choices=["", "a", "b", "c", "d", "e"])
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("--rounds >= 10 (20 timed calls per leg)")
    import torch
    from stellard_amd import build, verify as V
    from tests import datasets
    dev = torch.device("cuda", 0)
    out = {"tool": "sigcache_bench", "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
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
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

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
    nw = (n + 63) // 64
    half = n // 2
    out["rows"] = n
    out["blob_bytes"] = int(bp["total"])
    d_buf = torch.from_numpy(bp["buf"]).to(dev)
    d_off = torch.from_numpy(bp["offs"]).to(dev)
    d_len = torch.from_numpy(bp["lens"]).to(dev)
    ref = {"words": torch.empty(nw, dtype=torch.int64, device=dev),
           "status": torch.empty(n, dtype=torch.uint8, device=dev),
           "ids": torch.zeros((n, 32), dtype=torch.uint8, device=dev)}
    got = {"words": torch.empty(nw, dtype=torch.int64, device=dev),
           "status": torch.empty(n, dtype=torch.uint8, device=dev),
           "ids": torch.zeros((n, 32), dtype=torch.uint8, device=dev)}
    hit_words = torch.empty(nw, dtype=torch.int64, device=dev)
    cache = V.SigCache(args.sets_log2)
    out["cache"] = cache.info()

    def uncached():
        V.signed_blob_verify_batch_device(d_buf, d_off, d_len, out_words=ref["words"], out_status=ref["status"],
                                          out_ids=ref["ids"], stream=s)

    def cached(rows=n):
        o = cache.signed_blob_verify_batch_device(d_buf, d_off[:rows], d_len[:rows],
                                                  out_words=got["words"][: (rows + 63) // 64],
                                                  out_status=got["status"][:rows], out_ids=got["ids"][:rows], stream=s)
        return o["hits"], o["verified"]

    def same():
        torch.cuda.synchronize()
        return bool(torch.equal(ref["words"], got["words"]) and torch.equal(ref["status"], got["status"])
                    and torch.equal(ref["ids"], got["ids"]))

    def check():
        uncached()
        cold = cached()
        good = same()
        warm = cached()
        good = good and same()
        status = ref["status"].cpu().numpy()
        bits = V.words_to_bool(ref["words"], n)
        ok = status == V.TX_OK
        good = good and cold == (0, int(ok.sum())) and warm[0] + warm[1] == int(ok.sum())
        cache.lookup_device(ref["ids"], out_words=hit_words, stream=s)
        torch.cuda.synchronize()
        there = V.words_to_bool(hit_words, n)
        good = good and not bool((there & ~(bits & ok)).any())
        return good, {"tx_ok_rows": int(ok.sum()), "accepted": int(bits.sum()), "present_after_one_pass": int(there.sum())}
    good, counts = step("check", check)
    out["outputs_checked"] = good
    out.update(counts)
    if not good:
        print(json.dumps(out))
        print("the cached call's outputs are wrong", file=sys.stderr)
        sys.exit(1)

    def prepare(leg):
        """What is not timed: the state of the cache before the leg's call."""
        if leg in ("b", "d"):
            cache.clear(s)
        if leg == "d":
            cached(half)
        torch.cuda.synchronize()

    run = {"a": uncached, "b": cached, "c": cached, "d": cached,
           "e": lambda: cache.lookup_device(ref["ids"], out_words=hit_words, stream=s)}
    names = {"a": "a_uncached", "b": "b_cold", "c": "c_warm", "d": "d_half_seen", "e": "e_lookup"}

    def legs():
        ts = {k: [] for k in run}
        counts = {}
        uncached()
        cached()
        cached()  # the cache is warm, every buffer has its size
        torch.cuda.synchronize()
        order = [args.only] * 2 if args.only else list(run) + list(run)[::-1]
        for _ in range(args.rounds):
            for k in order:
                prepare(k)
                ms, r = timed(run[k])
                ts[k].append(ms)
                if k in "bcd":
                    counts[k] = r  # (b's and d's own inserts leave the cache warm for c)
        return ts, counts
    ts, counts = step("legs", legs)
    out["legs"] = {names[k]: spread(v) for k, v in ts.items() if v}
    for k, (hits, verified) in counts.items():
        out["legs"][names[k]].update(hits=int(hits), verified=int(verified))
    med = {k: v["median_ms"] for k, v in out["legs"].items()}
    if "a_uncached" in med:
        for k in med:
            if k != "a_uncached":
                out[k + "_over_a"] = round(med[k] / med["a_uncached"], 4)
        if "b_cold" in med:
            out["cold_price"] = round(med["b_cold"] / med["a_uncached"] - 1, 4)
    cache.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
