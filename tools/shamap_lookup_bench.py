"""What the resident SHAMap's read-only calls cost, device-resident, on one GPU.

    (a) stl_shamap_tree_lookup_device of 2^20 queries against a tree of 2^20
        uniformly random keys -- every query present, every query absent, half
        each -- and the same against 3 * 2^22 keys (--no-large leaves that out)
    (b) the same lookups with the bucket step off (STL_TUNE_SHAMAP_LOOKUP_BUCKETS
        0: the whole array is bisected), alternating call by call with (a), so
        the bucket-directed search is judged by its own A/B run
    (c) stl_shamap_tree_compare_device of two 2^20-key trees that differ by 0,
        4,096 and 65,536 rows (half replaces, three eighths inserts, one eighth
        deletes: one apply's batch) and in every leaf hash, with counts[4..5]
        (buckets and items examined) beside each time

Per case two warm-up calls (the workspaces have their size), then --calls timed
calls, each between two device events: median, min, max.  Before timing, a lookup
and a compare on a 2^16-key pair are checked against the Python model
(tests/shamap_lookup_py.py).  Prints one JSON line (kept as
profiles/shamap_lookup/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_lookup_bench.py [--calls C] [--no-large] [--step-timeout S] [--out FILE]
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
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from stellard_amd import _native as N, build, verify as V
    from tests import shamap_lookup_py as LM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_lookup_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "source_digest": build.source_digest()[:16], "lookup": {}, "compare": {}}

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

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def buckets(on):
        return N.load().stl_debug_tuning(N.STL_TUNE_SHAMAP_LOOKUP_BUCKETS, 1 if on else 0)

    step("init", V.init)
    s = torch.cuda.current_stream()
    gen = torch.Generator(device=dev)
    gen.manual_seed(2025)

    def rand_rows(n):
        return torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)

    # the model's word first
    def model_check():
        rng = np.random.default_rng(31)
        base = {k: v for k, v in zip(LM._rand(rng, 1 << 16), LM._rand(rng, 1 << 16))}
        a, b = LM.derive(base, rng, 300, 400, 500)
        probes = list(a)[:3000] + LM._rand(rng, 1000)
        ok = True
        with V.ShamapTree(1 << 17) as ta, V.ShamapTree(1 << 17) as tb:
            for t, items in ((ta, a), (tb, b)):
                t.apply_device(*[on_device(x) for x in LM.arrays(items)], stream=s)
            for on in (True, False):
                buckets(on)
                words, leaf, pos = ta.lookup_device(on_device(np.frombuffer(b"".join(probes), np.uint8).reshape(-1, 32)),
                                                    leaf_hashes=True, positions=True, stream=s)
                torch.cuda.synchronize()
                bits = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:len(probes)]
                wf, wl, wp = LM.lookup(a, probes)
                ok = ok and bits.astype(bool).tolist() == wf and leaf.cpu().numpy().tobytes() == b"".join(wl) and \
                    pos.cpu().numpy().view(np.uint32).tolist() == wp
            buckets(True)
            d = ta.compare_device(tb, max_rows=2048, stream=s)
            torch.cuda.synchronize()
            rows, counts = LM.compare(a, b, 2048)
            r = d.rows()
            ok = ok and [int(x) for x in d.counts.cpu().numpy()] == counts and r == len(rows) and \
                d.key[:r].cpu().numpy().tobytes() == b"".join(x[0] for x in rows) and \
                d.kind[:r].cpu().numpy().tolist() == [x[1] for x in rows] and \
                d.leaf_a[:r].cpu().numpy().tobytes() == b"".join(x[2] for x in rows) and \
                d.leaf_b[:r].cpu().numpy().tobytes() == b"".join(x[3] for x in rows)
        return ok
    out["model_checked"] = step("model", model_check)
    if not out["model_checked"]:
        print(json.dumps(out))
        print("the 2^16 pair differs from the model's", file=sys.stderr)
        sys.exit(1)

    def lookups(name, m, capacity):
        keys = rand_rows(m)
        rec = {"items": int(m), "queries": 1 << 20, "cases": {}}
        n = 1 << 20
        words = torch.zeros(n // 64, dtype=torch.int64, device=dev)
        leaf = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        pos = torch.zeros(n, dtype=torch.int32, device=dev)
        with V.ShamapTree(capacity) as tree:
            step(name + " load", lambda: tree.apply_device(keys, None, None, stream=s))
            present = keys[torch.randint(0, m, (n,), device=dev, generator=gen)].contiguous()
            absent = rand_rows(n)
            half = torch.cat([present[:n // 2], absent[:n // 2]])[torch.randperm(n, device=dev, generator=gen)].contiguous()
            for case, q, want in (("all_present", present, n), ("all_absent", absent, 0), ("half", half, n // 2)):
                def legs():
                    t = {True: [], False: []}
                    found = {}
                    for i in range(args.calls + 2):
                        for on in (True, False):  # the A/B legs alternate call by call
                            buckets(on)
                            ms = timed(lambda: tree.lookup_device(q, out_words=words, leaf_hashes=leaf, positions=pos,
                                                                  stream=s))
                            if i >= 2:
                                t[on].append(ms)
                            found[on] = int(torch.count_nonzero(pos != -1))
                    buckets(True)
                    bits_only = [timed(lambda: tree.lookup_device(q, out_words=words, stream=s))
                                 for _ in range(args.calls + 2)][2:]
                    hits = int(torch.count_nonzero(pos != -1))
                    return t, found, bits_only, hits
                try:
                    t, found, bits_only, hits = step(f"{name} {case}", legs)
                finally:
                    buckets(True)
                r = {"found": hits, "found_as_expected": hits == want and found[True] == found[False],
                     "by_bucket": spread(t[True]), "whole_array": spread(t[False]),
                     "by_bucket_bits_only": spread(bits_only)}
                r["whole_over_bucket"] = round(r["whole_array"]["median_ms"] / r["by_bucket"]["median_ms"], 2)
                r["queries_per_s_by_bucket"] = round(n / (r["by_bucket"]["median_ms"] * 1e-3))
                rec["cases"][case] = r
        out["lookup"][name] = rec

    def compares():
        m = 1 << 20
        keys, lh = rand_rows(m), rand_rows(m)
        rec = {"items": m, "cases": {}}
        cnt = torch.zeros(8, dtype=torch.int32, device=dev)
        with V.ShamapTree(m + (1 << 17)) as ta:
            step("compare load", lambda: ta.apply_device(keys, lh, None, stream=s))
            for case, rows in (("0", 0), ("4096", 4096), ("65536", 65536), ("every_leaf_hash", m)):
                with V.ShamapTree(m + (1 << 17)) as tb:
                    def build():
                        tb.apply_device(keys, lh, None, stream=s)
                        if rows == m:
                            tb.apply_device(keys, rand_rows(m), None, stream=s)
                        elif rows:
                            nrep, ndel = rows // 2, rows // 8
                            perm = torch.randperm(m, device=dev, generator=gen)[:nrep + ndel]
                            k = torch.cat([keys[perm], rand_rows(rows - nrep - ndel)])
                            op = torch.zeros(rows, dtype=torch.uint8, device=dev)
                            op[nrep:nrep + ndel] = 1
                            tb.apply_device(k.contiguous(), rand_rows(rows), op, stream=s)
                        ta.info(), tb.info()  # the hosts' bounds of the counts are exact: the slots are sized by them
                    step(f"compare {case} build", build)
                    room = max(rows, 1)
                    diff = V.DeviceDiff(room, counts=cnt)

                    def legs():
                        return [timed(lambda: ta.compare_device(tb, diff=diff, stream=s))
                                for _ in range(args.calls + 2)][2:]
                    t = step(f"compare {case}", legs)
                    c = [int(x) for x in cnt.cpu().numpy()]
                    r = {"differences": c[0], "a_only": c[1], "b_only": c[2], "changed": c[3],
                         "buckets_examined": c[4], "items_examined": c[5], "items_a": c[6], "items_b": c[7],
                         "differences_as_expected": c[0] == rows, "compare": spread(t)}
                    # the rows are in key order
                    w = min(c[0], room)
                    if w > 1:
                        kk = diff.key[:w].cpu().numpy()
                        order = [kk[i].tobytes() for i in range(0, w, max(w // 4096, 1))]
                        r["rows_ascend"] = all(x < y for x, y in zip(order, order[1:]))
                    rec["cases"][case] = r
        out["compare"] = rec

    lookups("tree_2^20", 1 << 20, (1 << 20) + (1 << 17))
    if not args.no_large:
        lookups("tree_large", 3 << 22, 1 << 24)
    compares()
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shamap_tree",
                       "bench.json")
    if os.path.exists(ref):  # the parent's recorded figures, for scale
        with open(ref) as f:
            b = json.load(f)["trees"]["tree_2^20"]["batches"]["4096"]
        out["reference"] = {"source": "profiles/shamap_tree/bench.json", "apply_4096_on_2^20_median_ms":
                            b["apply"]["median_ms"], "full_rebuild_2^20_median_ms": b["full_rebuild"]["median_ms"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
