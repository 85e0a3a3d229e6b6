"""What a fetch pack between two resident SHAMaps
(stl_shamap_tree_fetch_pack_device) costs, device-resident, on one GPU.

    (a) forked     2^20 keys; want = have forked with 256, 4,096 and 65,536 rows
                   (half replaces of resident keys, three eighths inserts, one
                   eighth deletes, every call a batch of its own).  The fetch
                   pack alternates with the only exact route there was before --
                   stl_shamap_tree_export_device of want, then
                   stl_shamap_nodes_device over the export (its row count read
                   outside the timed part) -- the order within a pair
                   alternating.  Beside both: stl_shamap_tree_fork_nodes_device
                   of the same batch, which gives the superset E and does the
                   apply as well.  Then, with stl_set_phase_timing on, the
                   library's marks: buckets and gather, levels, top and finish.
    (b) none       have NULL on 2^20 keys against export plus nodes
    (c) identical  want a snapshot of have: the floor -- buckets, two top folds,
                   the finish
    (d) large      12,582,912 keys (capacity 2^24), 4,096 rows

Per leg two warm-up calls, then 20 timed calls, each between two device events
(median, min, max).  Before timing, the pack of a 2^16-key tree against its fork
by a 4,096-row batch is checked against the Python model
(tests/shamap_fetch_py.py).  Prints one JSON line (kept as
profiles/shamap_fetch/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_fetch_bench.py [--calls C] [--no-large] [--step-timeout S] [--out FILE]
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
    from tests import shamap_fetch_py as FP, shamap_nodes_py as NM, shamap_py as SM, shamap_tree_py as TM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_fetch_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
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
    cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    fcnt = torch.zeros(8, dtype=torch.int32, device=dev)
    ncnt = torch.zeros(4, dtype=torch.int32, device=dev)
    items = torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2026)

    # the model's word first
    def model_check():
        k16 = SM.case_keys("random65536", 16)
        have_items = {k.tobytes(): k.tobytes() for k in k16}
        batch = TM._mixed_batch(np.random.default_rng(17), have_items, 4096)
        m = TM.Model()
        m.items = dict(have_items)
        m.apply(*batch)
        ok = True
        with V.ShamapTree(1 << 16) as have, V.ShamapTree(1 << 17) as want:
            have.apply_device(on_device(k16), stream=s)
            have.fork_device(want, *[on_device(x) for x in batch], stream=s)
            for hv_tree, hv in ((have, have_items), (None, None)):
                pack = FP.pack_by_difference(m.items, hv)
                nodes, c = want.fetch_pack_device(hv_tree, max_nodes=len(pack) + 1, counts=True, stream=s)
                torch.cuda.synchronize()
                got = NM.rows_as_dict(nodes.rows(), nodes.hash.cpu().numpy(), nodes.body.cpu().numpy(),
                                      nodes.ids.cpu().numpy(), nodes.meta.cpu().numpy())
                ok = ok and got == pack and [int(x) for x in c.cpu()] == FP.counts(m.items, hv, pack)
        return ok
    out["model_checked"] = step("model", model_check)
    if not out["model_checked"]:
        fail("the 2^16 tree's fetch pack differs from the model's")

    def loaded(keys, capacity):
        t = V.ShamapTree(capacity)
        t.apply_device(keys, None, None, out_root=root, counts=cnt, stream=s)
        assert t.info()["items"] == keys.shape[0]  # the host's bound of the count is exact
        return t

    def make_batch(keys, rows):
        m = keys.shape[0]
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

    def trees(name, m, capacity, batch_rows, route, node_room):
        """have of m keys; per batch size: want = have forked, the pack timed."""
        keys = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        have, want = loaded(keys, capacity), V.ShamapTree(capacity)
        e_nodes, f_nodes = V.DeviceNodes(node_room), V.DeviceNodes(node_room)
        r_nodes = V.DeviceNodes(node_room) if route else None
        ek = torch.empty((capacity, 32), dtype=torch.uint8, device=dev) if route else None
        el = torch.empty((capacity, 32), dtype=torch.uint8, device=dev) if route else None
        rec = {"items": m, "capacity": capacity, "node_room": node_room, "batches": {}}

        def fetch(hv):
            return lambda: want.fetch_pack_device(hv, nodes=f_nodes, counts=fcnt, stream=s)

        def export_nodes(n):
            def go():
                want.export_device(ek, el, items, stream=s)
                V.shamap_nodes_device(ek[:n], el[:n], nodes=r_nodes, out_root=root, counts=ncnt, stream=s)
            return go

        def pair(first, second):
            return timed(first), timed(second)

        try:
            for rows in batch_rows:
                def legs():
                    tf, tr, te, ok, last = [], [], [], True, None
                    place = {"fetch_first": [], "fetch_second": [], "route_first": [], "route_second": []}
                    for i in range(args.calls + 2):
                        if rows:
                            bt = make_batch(keys, rows)
                            torch.cuda.synchronize()
                            t3 = timed(lambda: have.fork_nodes_device(want, *bt, nodes=e_nodes, out_root=root,
                                                                      counts=cnt, stream=s))
                        else:
                            t3 = timed(lambda: have.fork_nodes_device(want, nodes=e_nodes, out_root=root, counts=cnt,
                                                                      stream=s))
                        n = int(cnt[0])  # waits, outside the timed parts
                        torch.cuda.synchronize()
                        if route:
                            if i % 2 == 0:  # the order alternates: a pair's first call starts on an idle device
                                t1, t2 = pair(fetch(have), export_nodes(n))
                            else:
                                t2, t1 = pair(export_nodes(n), fetch(have))
                        else:
                            t1, t2 = timed(fetch(have)), None
                        c = [int(x) for x in fcnt.cpu().numpy()]
                        ok = ok and c[4] - c[5] == c[0] == int(f_nodes.count.item()) <= node_room and c[6] == n
                        ok = ok and (not rows or c[0] <= int(e_nodes.count.item()))
                        if route:
                            ok = ok and c[0] <= int(r_nodes.count.item()) <= node_room
                        if i >= 2:
                            tf.append(t1)
                            te.append(t3)
                            if route:
                                tr.append(t2)
                                place["fetch_first" if i % 2 == 0 else "fetch_second"].append(t1)
                                place["route_second" if i % 2 == 0 else "route_first"].append(t2)
                            last = {"counts": c, "fork_nodes": int(e_nodes.count.item()),
                                    "all_nodes": int(r_nodes.count.item()) if route else None}
                    phases = []
                    was = V.set_phase_timing(True)
                    try:
                        for _ in range(args.calls):
                            torch.cuda.synchronize()
                            V.reset_stats()
                            fetch(have)()
                            torch.cuda.synchronize()
                            st = V.get_stats()
                            if st["phase_chunks"] == 1:
                                phases.append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
                    finally:
                        V.set_phase_timing(was)
                    return tf, tr, te, ok, last, phases, place
                tf, tr, te, ok, last, phases, place = step(f"{name} batch {rows}", legs)
                r = {"rows": rows, "consistent": ok, "last": last, "fetch_pack": spread(tf), "fork_nodes": spread(te)}
                if tr:
                    r["export_plus_nodes"] = spread(tr)
                    r["by_place_in_pair"] = {k: spread(v) for k, v in place.items() if v}
                    r["route_over_fetch"] = round(r["export_plus_nodes"]["median_ms"] / r["fetch_pack"]["median_ms"], 2)
                if phases:
                    r["fetch_phases"] = {p: spread([x[i] for x in phases])
                                         for i, p in enumerate(("buckets_gather", "levels", "top_finish"))}
                rec["batches"][str(rows)] = r
                if not ok:
                    out.setdefault("forked", {})[name] = rec
                    fail(f"{name} batch {rows}: the counts disagree")
            if route:  # (b) against none
                def none_legs():
                    tf, tr, ok = [], [], True
                    n = want.info()["items"]
                    for i in range(args.calls + 2):
                        torch.cuda.synchronize()
                        if i % 2 == 0:
                            t1, t2 = pair(fetch(None), export_nodes(n))
                        else:
                            t2, t1 = pair(export_nodes(n), fetch(None))
                        ok = ok and int(f_nodes.count.item()) == int(r_nodes.count.item()) <= node_room
                        if i >= 2:
                            tf.append(t1)
                            tr.append(t2)
                    return tf, tr, ok, int(f_nodes.count.item())
                tf, tr, ok, nodes = step(f"{name} against none", none_legs)
                rec["against_none"] = {"nodes": nodes, "counts_agree": ok, "fetch_pack": spread(tf),
                                       "export_plus_nodes": spread(tr)}
                if not ok:
                    out.setdefault("forked", {})[name] = rec
                    fail(f"{name}: against none the pack is not every node")
        finally:
            have.close()
            want.close()
        out.setdefault("forked", {})[name] = rec
        return rec

    cap20 = (1 << 20) + (1 << 18)
    f20 = trees("tree_2^20", 1 << 20, cap20, (256, 4096, 65536, 0), True, 1 << 20)
    out["identical"] = f20["batches"].pop("0")  # (c): want a snapshot of have
    if not args.no_large:
        trees("tree_large", 3 << 22, 1 << 24, (4096,), False, 1 << 19)

    r = f20["batches"]["4096"]
    out["condition"] = {"tree": "tree_2^20", "rows": 4096, "fetch_pack_max_ms": r["fetch_pack"]["max_ms"],
                        "export_plus_nodes_min_ms": r["export_plus_nodes"]["min_ms"],
                        "met": r["fetch_pack"]["max_ms"] < r["export_plus_nodes"]["min_ms"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
