"""What one apply to a resident SHAMap (stl_shamap_tree_apply_device) costs,
device-resident, on one GPU, next to the only other way to the same root: the
full rebuild, stl_shamap_root_device over the tree's whole exported content.

    tree_2^20        2^20 uniformly random keys
    tree_large       3 * 2^22 uniformly random keys in a tree of capacity 2^24
                     (STL_SHAMAP_MAX_ITEMS bounds the capacity, and the inserts need room)
    clustered_2^20   2^20 keys in 4,096 clusters that share 40 nibbles

and for each tree batches of 256, 4,096 and 65,536 rows (the clustered tree:
4,096): half replaces of resident keys, three eighths inserts of new random
keys, one eighth deletes of resident keys, every call a batch of its own.  Per
(tree, batch) 20 applies, each between two device events, alternating with 20
full rebuilds over the content exported after that apply (median, min, max; the
two roots must agree every time).  Then, in calls of their own with
stl_set_phase_timing on, the library's own marks: locate (the batch's sort,
heads, compaction, bisection and scan), merge, subtrees (bounds, gather, the
neighbour and level launches) and top (bucket values, the four top launches and
the finish).  Before timing, root and counts of a 4,096-row batch on a 2^16-key
tree are checked against the Python model (tests/shamap_tree_py.py).  Prints one
JSON line (kept as profiles/shamap_tree/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_tree_bench.py [--calls C] [--no-large] [--step-timeout S] [--out FILE]
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
    from stellard_amd import build, verify as V
    from tests import shamap_py as SM, shamap_tree_py as TM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_tree_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "source_digest": build.source_digest()[:16], "trees": {}}

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

    step("init", V.init)
    s = torch.cuda.current_stream()
    root = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    full_root = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    full_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    items = torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024)

    # the model's word first
    def model_check():
        k16 = SM.case_keys("random65536", 16)
        batch = TM._mixed_batch(np.random.default_rng(17), {k.tobytes(): None for k in k16}, 4096)
        m = TM.Model()
        with V.ShamapTree(1 << 17) as t:
            got = []
            for b in ((k16, None, None), batch):
                want = m.apply(*b)
                t.apply_device(*[None if x is None else on_device(x) for x in b], out_root=root, counts=cnt, stream=s)
                torch.cuda.synchronize()
                got.append((root.cpu().numpy().tobytes(), [int(x) for x in cnt.cpu().numpy()]) == want)
        return all(got)
    out["model_checked"] = step("model", model_check)
    if not out["model_checked"]:
        print(json.dumps(out))
        print("the 2^16 tree differs from the model's", file=sys.stderr)
        sys.exit(1)

    def measure(name, keys, capacity, batch_rows):
        """keys: (m, 32) uint8 on the device, distinct; the tree is loaded by one apply."""
        m = keys.shape[0]
        rec = {"items_loaded": int(m), "capacity": int(capacity), "batches": {}}
        tree = V.ShamapTree(capacity)
        exp_k = torch.empty((capacity, 32), dtype=torch.uint8, device=dev)
        exp_l = torch.empty((capacity, 32), dtype=torch.uint8, device=dev)
        try:
            def load():
                return timed(lambda: tree.apply_device(keys, None, None, out_root=root, counts=cnt, stream=s))
            rec["load_ms"] = round(step(name + " load", load), 4)
            info = tree.info()
            assert info["items"] == m
            rec["bytes"] = int(info["bytes"])
            rec["bytes_per_row_of_capacity"] = round(info["bytes"] / capacity, 2)
            perm = torch.randperm(m, device=dev, generator=gen)
            used = 0  # rows of perm already deleted

            def make_batch(rows):
                nonlocal used
                nrep, ndel = rows // 2, rows // 8
                nins = rows - nrep - ndel
                dele = keys[perm[used:used + ndel]]
                used += ndel
                rep = keys[perm[used + torch.randint(0, m - used, (nrep,), device=dev, generator=gen)]]
                ins = torch.randint(0, 256, (nins, 32), dtype=torch.uint8, device=dev, generator=gen)
                k = torch.cat([rep, ins, dele])
                op = torch.cat([torch.zeros(nrep + nins, dtype=torch.uint8, device=dev),
                                torch.ones(ndel, dtype=torch.uint8, device=dev)])
                order = torch.randperm(rows, device=dev, generator=gen)
                lh = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
                return k[order].contiguous(), lh, op[order].contiguous()

            for rows in batch_rows:
                def apply(b):
                    tree.apply_device(*b, out_root=root, counts=cnt, stream=s)

                def rebuild():
                    V.shamap_root_device(exp_k[:now], exp_l[:now], None, out_root=full_root, counts=full_cnt, stream=s)

                def legs():
                    nonlocal now
                    tree.info()  # the host's bound of the count is exact again: no apply below waits
                    agree, ta, tr, counts = True, [], [], None
                    for i in range(args.calls + 2):  # two calls of each first: the workspaces have their size
                        b = make_batch(rows)
                        torch.cuda.synchronize()
                        t = timed(lambda: apply(b))
                        tree.export_device(exp_k, exp_l, items, stream=s)
                        torch.cuda.synchronize()
                        now = int(items[0])
                        t2 = timed(rebuild)
                        agree = agree and bool((root == full_root).all()) and int(cnt[0]) == now == int(full_cnt[0])
                        if i >= 2:
                            ta.append(t)
                            tr.append(t2)
                            counts = [int(x) for x in cnt.cpu().numpy()]
                    was = V.set_phase_timing(True)
                    phases = []
                    try:
                        for _ in range(args.calls):
                            b = make_batch(rows)
                            torch.cuda.synchronize()
                            V.reset_stats()
                            apply(b)
                            torch.cuda.synchronize()
                            st = V.get_stats()
                            if st["phase_chunks"] == 1:
                                phases.append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
                    finally:
                        V.set_phase_timing(was)
                    return agree, ta, tr, counts, phases
                now = m
                agree, ta, tr, counts, phases = step(f"{name} batch {rows}", legs)
                r = {"rows": rows, "roots_agree": agree, "last_counts": counts, "items": now,
                     "apply": spread(ta), "full_rebuild": spread(tr)}
                r["rebuild_over_apply"] = round(r["full_rebuild"]["median_ms"] / r["apply"]["median_ms"], 2)
                r["apply_max_below_rebuild_min"] = r["apply"]["max_ms"] < r["full_rebuild"]["min_ms"]
                if phases:
                    for i, ph in enumerate(("locate", "merge", "subtrees", "top")):
                        r[ph] = spread([p[i] for p in phases])
                rec["batches"][str(rows)] = r
                if not agree:
                    out["trees"][name] = rec
                    print(json.dumps(out))
                    print(f"{name} batch {rows}: the apply's root differs from the full rebuild's", file=sys.stderr)
                    sys.exit(1)
        finally:
            tree.close()
        out["trees"][name] = rec
        return rec

    def distinct(keys):
        # (random 256-bit keys collide with probability 2^-200; clustered ones are random past nibble 40)
        return on_device(keys)

    measure("tree_2^20", distinct(SM.case_keys("random1048576", 20)), (1 << 20) + (1 << 22), (256, 4096, 65536))
    measure("clustered_2^20", distinct(SM.case_keys("cluster1048576_4096_40", 21)), (1 << 20) + (1 << 20), (4096,))
    if not args.no_large:
        big = torch.randint(0, 256, (3 << 22, 32), dtype=torch.uint8, device=dev, generator=gen)
        measure("tree_large", big, 1 << 24, (256, 4096, 65536))
    r = out["trees"]["tree_2^20"]["batches"]["4096"]
    out["done_condition"] = {"tree": "tree_2^20", "rows": 4096, "apply_max_ms": r["apply"]["max_ms"],
                             "full_rebuild_min_ms": r["full_rebuild"]["min_ms"],
                             "met": r["apply_max_below_rebuild_min"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
