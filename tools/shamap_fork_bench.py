"""What a fork of a resident SHAMap (stl_shamap_tree_fork_device) costs,
device-resident, on one GPU.

    (a) snapshot   trees of 2^20 keys and of 3 * 2^22 keys (capacity 2^24): the
                   fork of no rows, alternating with a device-to-device copy of
                   as many bytes (the floor) and with the only route there was
                   before -- stl_shamap_tree_export_device, then a load by apply
                   into an empty tree
    (b) fork       2^20 keys, batches of 256, 4,096 and 65,536 rows (half
                   replaces of resident keys, three eighths inserts of new random
                   keys, one eighth deletes of resident keys, every call a batch
                   of its own), alternating with stl_shamap_tree_apply_device of
                   the same batch on a tree of the same content (turned back by
                   stl_shamap_tree_revert after every call), the order within a
                   pair alternating (the first call of a pair starts on an idle
                   device: by_place_in_pair); the two roots must agree every
                   time.  Then, with stl_set_phase_timing on, the library's
                   marks of both: locate, merge, subtrees, top.
    (c) consensus  a 4,096-key transaction set forked with 8 changed rows

Per leg two warm-up calls, then 20 timed calls, each between two device events
(median, min, max).  Before timing, a fork of a 4,096-row batch and a snapshot
of a 2^16-key tree are checked against the Python model
(tests/shamap_fork_py.py).  Prints one JSON line (kept as
profiles/shamap_fork/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_fork_bench.py [--calls C] [--no-large] [--step-timeout S] [--out FILE]
"""
import argparse
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEN_FIXED_BYTES = 4 * 65536 + 32 * 65536 + 64  # a generation besides its rows: bucket values and meta words


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
    from tests import shamap_fork_py as FM, shamap_py as SM, shamap_tree_py as TM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_fork_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
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

    def on_device(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def fail(msg):
        print(json.dumps(out))
        print(msg, file=sys.stderr)
        sys.exit(1)

    step("init", V.init)
    s = torch.cuda.current_stream()
    root = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    root2 = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    cnt2 = torch.zeros(8, dtype=torch.int32, device=dev)
    items = torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2025)

    # the model's word first
    def model_check():
        k16 = SM.case_keys("random65536", 16)
        m = TM.Model()
        m.apply(k16)
        batch = TM._mixed_batch(np.random.default_rng(17), m.items, 4096)
        ok = True
        with V.ShamapTree(1 << 16) as src, V.ShamapTree(1 << 17) as dst:
            src.apply_device(on_device(k16), stream=s)
            for b in ((None, None, None), batch):
                want, wroot, wcounts = FM.fork(m, *b)
                src.fork_device(dst, *[on_device(x) for x in b], out_root=root, counts=cnt, stream=s)
                ek = torch.empty((1 << 17, 32), dtype=torch.uint8, device=dev)
                el = torch.empty((1 << 17, 32), dtype=torch.uint8, device=dev)
                dst.export_device(ek, el, items, stream=s)
                torch.cuda.synchronize()
                now = int(items[0])
                wk, wl = want.content()
                ok = ok and (root.cpu().numpy().tobytes(), [int(x) for x in cnt.cpu().numpy()]) == (wroot, wcounts)
                ok = ok and now == len(want.items) and ek[:now].cpu().numpy().tobytes() == wk.tobytes() \
                    and el[:now].cpu().numpy().tobytes() == wl.tobytes()
            ok = ok and src.info()["root"] == m.root() and src.info()["items"] == 65536
        return ok
    out["model_checked"] = step("model", model_check)
    if not out["model_checked"]:
        fail("the 2^16 tree's fork differs from the model's")

    def loaded(keys, capacity):
        t = V.ShamapTree(capacity)
        t.apply_device(keys, None, None, out_root=root, counts=cnt, stream=s)
        assert t.info()["items"] == keys.shape[0]  # the host's bound of the count is exact
        return t

    # ---- (a) the snapshot ----
    def snapshot(name, m, capacity):
        keys = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        src, dst, ld = loaded(keys, capacity), V.ShamapTree(capacity), V.ShamapTree(capacity)
        nbytes = 64 * m + GEN_FIXED_BYTES
        a, b = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ek = torch.empty((m, 32), dtype=torch.uint8, device=dev)
        el = torch.empty((m, 32), dtype=torch.uint8, device=dev)
        try:
            def export_load():
                src.export_device(ek, el, items, stream=s)
                ld.apply_device(ek, el, None, out_root=root2, counts=cnt2, stream=s)

            def legs():
                ts, tc, te, agree = [], [], [], True
                for i in range(args.calls + 2):
                    torch.cuda.synchronize()
                    t1 = timed(lambda: src.fork_device(dst, out_root=root, counts=cnt, stream=s))
                    t2 = timed(lambda: b.copy_(a))
                    t3 = timed(export_load)
                    agree = agree and bool((root == root2).all()) and int(cnt[0]) == m == int(cnt2[0])
                    ld.revert()  # empty again, on the host alone
                    if i >= 2:
                        ts.append(t1)
                        tc.append(t2)
                        te.append(t3)
                return ts, tc, te, agree and dst.info()["root"] == src.info()["root"]
            ts, tc, te, agree = step(name, legs)
        finally:
            for t in (src, dst, ld):
                t.close()
        r = {"items": m, "capacity": capacity, "bytes_copied": nbytes, "roots_agree": agree, "snapshot": spread(ts),
             "device_copy": spread(tc), "export_then_load": spread(te)}
        r["snapshot_over_copy"] = round(r["snapshot"]["median_ms"] / r["device_copy"]["median_ms"], 2)
        r["export_then_load_over_snapshot"] = round(r["export_then_load"]["median_ms"] / r["snapshot"]["median_ms"], 2)
        r["snapshot_GBps_read_plus_written"] = round(2 * nbytes / r["snapshot"]["median_ms"] / 1e6, 1)
        out.setdefault("snapshot", {})[name] = r
        if not agree:
            fail(f"{name}: the snapshot's root differs from the load's")
        return r

    snap20 = snapshot("tree_2^20", 1 << 20, (1 << 20) + (1 << 18))
    if not args.no_large:
        snapshot("tree_large", 3 << 22, 1 << 24)

    # ---- (b) the fork with rows, next to the apply ----
    def forks(name, m, capacity, batch_rows):
        keys = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        src, twin, dst = loaded(keys, capacity), loaded(keys, capacity), V.ShamapTree(capacity)
        rec = {"items": m, "capacity": capacity, "batches": {}}

        def make_batch(rows):
            nrep, ndel = rows // 2, rows // 8
            nins = rows - nrep - ndel
            pick = torch.randperm(m, device=dev, generator=gen)[:nrep + ndel]
            ins = torch.randint(0, 256, (nins, 32), dtype=torch.uint8, device=dev, generator=gen)
            k = torch.cat([keys[pick[:nrep]], ins, keys[pick[nrep:]]])
            op = torch.cat([torch.zeros(nrep + nins, dtype=torch.uint8, device=dev),
                            torch.ones(ndel, dtype=torch.uint8, device=dev)])
            order = torch.randperm(rows, device=dev, generator=gen)
            lh = torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
            return k[order].contiguous(), lh, op[order].contiguous()

        try:
            for rows in batch_rows:
                def legs():
                    tf, ta, agree, counts = [], [], True, None
                    place = {"fork_first": [], "fork_second": [], "apply_first": [], "apply_second": []}
                    for i in range(args.calls + 2):
                        bt = make_batch(rows)
                        fork = lambda: src.fork_device(dst, *bt, out_root=root, counts=cnt, stream=s)  # noqa: E731
                        apply = lambda: twin.apply_device(*bt, out_root=root2, counts=cnt2, stream=s)  # noqa: E731
                        torch.cuda.synchronize()
                        if i % 2 == 0:  # the pair's order alternates: the first call of a pair starts on an idle device
                            t1 = timed(fork)
                            t2 = timed(apply)
                        else:
                            t2 = timed(apply)
                            t1 = timed(fork)
                        agree = agree and bool((root == root2).all()) and bool((cnt == cnt2).all())
                        twin.revert()  # the same content again, and the bound that went with it
                        if i >= 2:
                            tf.append(t1)
                            ta.append(t2)
                            place["fork_first" if i % 2 == 0 else "fork_second"].append(t1)
                            place["apply_second" if i % 2 == 0 else "apply_first"].append(t2)
                            counts = [int(x) for x in cnt.cpu().numpy()]
                    was = V.set_phase_timing(True)
                    phases = {"fork": [], "apply": []}
                    try:
                        for _ in range(args.calls):
                            bt = make_batch(rows)
                            for leg in ("fork", "apply"):
                                torch.cuda.synchronize()
                                V.reset_stats()
                                if leg == "fork":
                                    src.fork_device(dst, *bt, out_root=root, counts=cnt, stream=s)
                                else:
                                    twin.apply_device(*bt, out_root=root2, counts=cnt2, stream=s)
                                torch.cuda.synchronize()
                                st = V.get_stats()
                                if st["phase_chunks"] == 1:
                                    phases[leg].append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
                            twin.revert()
                    finally:
                        V.set_phase_timing(was)
                    return tf, ta, agree, counts, phases, place
                tf, ta, agree, counts, phases, place = step(f"{name} batch {rows}", legs)
                r = {"rows": rows, "roots_agree": agree, "last_counts": counts, "fork": spread(tf), "apply": spread(ta)}
                r["by_place_in_pair"] = {k: spread(v) for k, v in place.items() if v}
                r["fork_over_apply"] = round(r["fork"]["median_ms"] / r["apply"]["median_ms"], 3)
                r["fork_median_within_apply_band"] = r["apply"]["min_ms"] <= r["fork"]["median_ms"] <= r["apply"]["max_ms"]
                for leg, ph in phases.items():
                    if ph:
                        r[leg + "_phases"] = {p: spread([x[i] for x in ph])
                                              for i, p in enumerate(("locate", "merge", "subtrees", "top"))}
                rec["batches"][str(rows)] = r
                if not agree:
                    out["fork"] = {name: rec}
                    fail(f"{name} batch {rows}: the fork's root or counts differ from the apply's")
        finally:
            for t in (src, twin, dst):
                t.close()
        out.setdefault("fork", {})[name] = rec
        return rec

    f20 = forks("tree_2^20", 1 << 20, (1 << 20) + (1 << 18), (256, 4096, 65536))

    # ---- (c) a consensus round ----
    def consensus():
        ids = torch.randint(0, 256, (4096, 32), dtype=torch.uint8, device=dev, generator=gen)
        acquired, position = loaded(ids, 8192), V.ShamapTree(8192)
        try:
            ts = []
            for i in range(args.calls + 2):
                flip = torch.cat([ids[torch.randperm(4096, device=dev, generator=gen)[:4]],
                                  torch.randint(0, 256, (4, 32), dtype=torch.uint8, device=dev, generator=gen)])
                op = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0], dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                t = timed(lambda: acquired.fork_device(position, flip, None, op, out_root=root, counts=cnt, stream=s))
                if i >= 2:
                    ts.append(t)
            ok = [int(x) for x in cnt.cpu().numpy()][:5] == [4096, 4, 0, 4, 0] and acquired.info()["items"] == 4096
            return ts, ok
        finally:
            acquired.close()
            position.close()
    ts, ok = step("consensus", consensus)
    out["consensus_round"] = {"items": 4096, "rows": 8, "counts_as_expected": ok, "fork": spread(ts)}

    r = f20["batches"]["4096"]
    out["condition"] = {"tree": "tree_2^20", "rows": 4096, "fork_max_ms": r["fork"]["max_ms"],
                        "export_then_load_min_ms": snap20["export_then_load"]["min_ms"],
                        "met": r["fork"]["max_ms"] < snap20["export_then_load"]["min_ms"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
