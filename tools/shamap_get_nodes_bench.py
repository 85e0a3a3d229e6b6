"""What a resident SHAMap's answers by node ID (stl_shamap_tree_get_nodes_device)
cost, device-resident, on one GPU.

    (a) 2^20 keys   1, 256 and 4,096 FAT requests at IDs drawn from existing
                    inner nodes at depths 0-6, and 4,096 PATH requests of
                    present keys.  Beside each, in the same run and the order
                    within a pair alternating, the only route there was before:
                    stl_shamap_tree_fetch_pack_device(tree, NULL), every inner
                    node of the tree -- its search on the host for the nodes
                    asked for is left out of the timed part, which favours it.
                    Then, with stl_set_phase_timing on, the library's marks:
                    ranges, tasks and gather; the levels; top and finish.
    (b) large       the 256-request case on 12,582,912 keys (capacity 2^24); the
                    old route stores only its first 2^19 nodes there

The one-request time is the call's floor: three scans, 61 + 60 level launches
and the top, whatever is asked.

Per leg two warm-up calls, then 20 timed calls, each between two device events
(median, min, max).  Before timing, 1,000 generated requests against a
2^16-key tree are checked against the Python model (tests/shamap_get_py.py).
Prints one JSON line (kept as profiles/shamap_get_nodes/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_get_nodes_bench.py [--calls C] [--no-large] [--step-timeout S] [--out FILE]
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
    from tests import shamap_get_py as GM, shamap_nodes_py as NM, shamap_py as SM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_get_nodes_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(2027)
    rng = np.random.default_rng(2027)

    # the model's word first
    def model_check():
        k16 = SM.case_keys("random65536", 16)
        items = {k.tobytes(): k[::-1].tobytes() for k in k16}
        requests = GM.requests_for(items, np.random.default_rng(18), 1000)
        ans = GM.Answer(items, requests)
        rid, rdepth, rmode = GM.request_arrays(requests)
        c = lambda t: t.cpu().numpy()  # noqa: E731
        with V.ShamapTree(1 << 16) as t:
            t.apply_device(on_device(k16), on_device(k16[:, ::-1]), stream=s)
            a = t.get_nodes_device(on_device(rid), on_device(rdepth), on_device(rmode), max_nodes=ans.total,
                                   counts=True, stream=s)
            torch.cuda.synchronize()
            try:
                GM.check_outputs(ans, c(a.status), c(a.first), c(a.rows), c(a.leaf_key), c(a.leaf_hash),
                                 c(a.nodes.hash), c(a.nodes.body), c(a.nodes.ids), c(a.nodes.meta),
                                 int(a.nodes.count.item()), c(a.counts))
            except AssertionError as e:
                print("model check:", e, file=sys.stderr)
                return False
        return True
    out["model_checked"] = step("model", model_check)
    if not out["model_checked"]:
        fail("the 2^16 tree's answers differ from the model's")

    def inner_ids(sorted_keys, n, depths):
        """n IDs of existing inner nodes, the depths drawn evenly: key i lies
        under an inner node at depth d when it shares d nibbles with its successor."""
        l = NM._neighbours_np(sorted_keys)
        under = {d: np.nonzero(l >= d)[0] for d in set(depths)}
        ids, ds = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        for j in range(n):
            d = int(depths[j % len(depths)])
            cand = under[d]
            i = int(cand[rng.integers(0, len(cand))])
            ids[j] = np.frombuffer(NM.masked(sorted_keys[i].tobytes(), d), np.uint8)
            ds[j] = d
        return ids, ds

    def tree_runs(name, m, capacity, legs, route_room):
        keys = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        t = V.ShamapTree(capacity)
        t.apply_device(keys, None, None, stream=s)
        assert t.info()["items"] == m  # the host's bound of the count is exact
        ek = torch.empty((capacity, 32), dtype=torch.uint8, device=dev)
        t.export_device(ek, None, stream=s)
        torch.cuda.synchronize()
        sample = ek[:min(m, 1 << 20)].cpu().numpy()  # sorted: neighbours within the slice are neighbours
        del ek, keys
        route_nodes = V.DeviceNodes(route_room)
        rcnt = torch.zeros(8, dtype=torch.int32, device=dev)
        rec = {"items": m, "capacity": capacity, "route_node_room": route_room, "legs": {}}
        try:
            for leg, n, mode in legs:
                if mode == GM.FAT:
                    ids, ds = inner_ids(sample, n, list(range(7)))
                else:
                    ids, ds = sample[rng.integers(0, len(sample), n)], np.zeros(n, np.uint8)
                d_ids, d_ds = on_device(ids), on_device(ds)
                d_modes = torch.full((n,), mode, dtype=torch.uint8, device=dev)
                nodes = V.DeviceNodes(GM.MAX_ROWS * n)
                gcnt = torch.zeros(8, dtype=torch.int32, device=dev)

                def get():
                    return t.get_nodes_device(d_ids, d_ds, d_modes, nodes=nodes, counts=gcnt, stream=s)

                def route():
                    return t.fetch_pack_device(None, nodes=route_nodes, counts=rcnt, stream=s)

                def run():
                    tg, tr = [], []
                    for i in range(args.calls + 2):
                        torch.cuda.synchronize()
                        if i % 2 == 0:  # the order alternates: a pair's first call starts on an idle device
                            a, b = timed(get), timed(route)
                        else:
                            b, a = timed(route), timed(get)
                        if i >= 2:
                            tg.append(a)
                            tr.append(b)
                    phases = []
                    was = V.set_phase_timing(True)
                    try:
                        for _ in range(args.calls):
                            torch.cuda.synchronize()
                            V.reset_stats()
                            get()
                            torch.cuda.synchronize()
                            st = V.get_stats()
                            if st["phase_chunks"] == 1:
                                phases.append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
                    finally:
                        V.set_phase_timing(was)
                    return tg, tr, phases
                tg, tr, phases = step(f"{name} {leg}", run)
                c = [int(x) for x in gcnt.cpu().numpy()]
                r = {"requests": n, "mode": "FAT" if mode == GM.FAT else "PATH", "counts": c,
                     "all_nodes": int(rcnt[0]), "get_nodes": spread(tg), "fetch_pack_none": spread(tr)}
                r["route_over_get"] = round(r["fetch_pack_none"]["median_ms"] / r["get_nodes"]["median_ms"], 2)
                if phases:
                    r["get_phases"] = {p: spread([x[i] for x in phases])
                                       for i, p in enumerate(("ranges_tasks_gather", "levels", "top_finish"))}
                rec["legs"][leg] = r
                if c[0] != int(nodes.count.item()) or c[1] + c[2] + c[3] != n or c[7] != m:
                    out[name] = rec
                    fail(f"{name} {leg}: the counts disagree")
        finally:
            t.close()
        out[name] = rec
        return rec

    cap20 = (1 << 20) + (1 << 18)
    r20 = tree_runs("tree_2^20", 1 << 20, cap20, (("fat_1", 1, GM.FAT), ("fat_256", 256, GM.FAT),
                                                  ("fat_4096", 4096, GM.FAT), ("path_4096", 4096, GM.PATH)), 1 << 19)
    if not args.no_large:
        tree_runs("tree_large", 3 << 22, 1 << 24, (("fat_256", 256, GM.FAT),), 1 << 19)
    r = r20["legs"]["fat_256"]
    out["floor_ms"] = r20["legs"]["fat_1"]["get_nodes"]
    out["condition"] = {"tree": "tree_2^20", "requests": 256, "get_nodes_max_ms": r["get_nodes"]["max_ms"],
                        "fetch_pack_none_min_ms": r["fetch_pack_none"]["min_ms"],
                        "met": r["get_nodes"]["max_ms"] < r["fetch_pack_none"]["min_ms"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
