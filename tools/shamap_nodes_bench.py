"""What storing the inner nodes costs (stl_shamap_nodes_device,
stl_shamap_tree_apply_nodes_device), device-resident, on one GPU, next to the
call that computes the same root and stores nothing, on the same input in the
same run:

    random_2^20      2^20 uniformly random IDs
    clustered_2^20   2^20 IDs in 4,096 clusters that share 40 nibbles
    tree_2^20/4096   4,096-row applies (half replaces, three eighths inserts, one
                     eighth deletes) to two trees of 2^20 random keys that are
                     given the same batches: one through the plain apply, one
                     through the storing apply

For each input the whole call of either kind, alternating, 20 calls each
between two device events (median, min, max), and in calls of their own with
stl_set_phase_timing on the library's own levels mark (the set calls) or
subtrees and top marks (the applies).  Also the nodes written, their bytes at
580 B a node, and the floor that number of bytes sets: a device-to-device copy
of as many bytes on this box, measured the same way (`copy`), which reads and
writes each byte once where the call only writes it.  Before timing, the node
count, root and a sample of rows of a 2^16 set are checked against the Python
model (tests/shamap_nodes_py.py).  Prints one JSON line (kept as
profiles/shamap_nodes/bench.json).

Every step runs under its own time limit (--step-timeout seconds), kept by a
watchdog thread; on a shared machine also run the tool under an outer
`timeout -k`.

    python3 tools/shamap_nodes_bench.py [--calls C] [--step-timeout S] [--out FILE]
"""
import argparse
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NODE_BYTES = 580


def spread(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
            "max_ms": round(float(a.max()), 4), "calls": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from stellard_amd import build, verify as V
    from tests import shamap_nodes_py as NM, shamap_py as SM
    dev = torch.device("cuda", 0)
    out = {"tool": "shamap_nodes_bench", "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "source_digest": build.source_digest()[:16], "node_bytes": NODE_BYTES, "inputs": {}}

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

    def phase_runs(call, prepare=None):
        was = V.set_phase_timing(True)
        phases = []
        try:
            for _ in range(args.calls):
                arg = prepare() if prepare else None
                torch.cuda.synchronize()
                V.reset_stats()
                call(arg) if prepare else call()
                torch.cuda.synchronize()
                st = V.get_stats()
                if st["phase_chunks"] == 1:
                    phases.append([st["phase_ns"][k] / 1e6 for k in V.PHASES])
        finally:
            V.set_phase_timing(was)
        return phases

    def copy_floor(nodes):
        """A device-to-device copy of the bytes `nodes` nodes take."""
        src = torch.empty(max(nodes, 1) * NODE_BYTES, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        t = spread([timed(lambda: dst.copy_(src)) for _ in range(args.calls)])
        t["bytes"] = int(src.numel())
        t["gb_per_s_written"] = round(src.numel() / 1e6 / t["median_ms"], 1) if t["median_ms"] else None
        return t

    step("init", V.init)
    s = torch.cuda.current_stream()
    root = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    root2 = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int32, device=dev)
    cnt2 = torch.zeros(4, dtype=torch.int32, device=dev)

    # the model's word first
    def model_check():
        k16 = SM.case_keys("random65536", 16)
        want = NM.nodes_closed_arrays(SM.the_set(k16)[0])
        _, c, nodes = V.shamap_nodes_device(on_device(k16), max_nodes=len(want[0]), out_root=root, counts=cnt, stream=s)
        torch.cuda.synchronize()
        rows = nodes.rows()
        meta = nodes.meta[:rows].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        got = (meta & 0xFF, nodes.ids[:rows].cpu().numpy(), nodes.hash[:rows].cpu().numpy(),
               nodes.body[:rows].cpu().numpy(), meta >> 16)
        return int(nodes.count.item()) == len(want[0]) == int(c[2]) and NM.same_nodes(got, want) and \
            root.cpu().numpy().tobytes() == SM.model(k16)[0]
    out["model_checked"] = bool(step("model", model_check))
    if not out["model_checked"]:
        print(json.dumps(out))
        print("the 2^16 node set differs from the model's", file=sys.stderr)
        sys.exit(1)

    def measure_set(name, keys):
        def plain():
            V.shamap_root_device(keys, None, None, out_root=root, counts=cnt, stream=s)

        def legs():
            plain()
            torch.cuda.synchronize()
            total = int(cnt[2])
            nodes = V.DeviceNodes(total, device=dev)

            def storing():
                V.shamap_nodes_device(keys, None, None, nodes=nodes, out_root=root2, counts=cnt2, stream=s)
            for _ in range(2):  # the workspace has its size
                plain()
                storing()
            torch.cuda.synchronize()
            agree = bool((root == root2).all()) and bool((cnt == cnt2).all()) and int(nodes.count.item()) == total
            tp, te = [], []
            for _ in range(args.calls):
                tp.append(timed(plain))
                te.append(timed(storing))
            pp, pe = phase_runs(plain), phase_runs(storing)
            rec = {"rows": int(keys.shape[0]), "counts": [int(x) for x in cnt.cpu().numpy()], "nodes_written": total,
                   "bytes_written": total * NODE_BYTES, "agree_with_plain_call": agree,
                   "plain": spread(tp), "storing": spread(te)}
            if pp and pe:
                rec["plain_levels"] = spread([p[2] for p in pp])
                rec["storing_levels"] = spread([p[2] for p in pe])
            rec["copy"] = copy_floor(total)
            rec["storing_minus_plain_ms"] = round(rec["storing"]["median_ms"] - rec["plain"]["median_ms"], 4)
            rec["extra_over_copy"] = round(rec["storing_minus_plain_ms"] / rec["copy"]["median_ms"], 2)
            return rec
        out["inputs"][name] = step(name, legs)

    measure_set("random_2^20", on_device(SM.case_keys("random1048576", 20)))
    measure_set("clustered_2^20", on_device(SM.case_keys("cluster1048576_4096_40", 21)))

    def measure_tree(name, keys, capacity, rows):
        gen = torch.Generator(device=dev)
        gen.manual_seed(2025)
        m = keys.shape[0]
        a, b = V.ShamapTree(capacity), V.ShamapTree(capacity)
        cnt8, cnt8b = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
        try:
            def legs():
                a.apply_device(keys, None, None, out_root=root, counts=cnt8, stream=s)
                b.apply_device(keys, None, None, out_root=root2, counts=cnt8b, stream=s)
                torch.cuda.synchronize()
                perm = torch.randperm(m, device=dev, generator=gen)
                used = 0

                def make_batch():
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

                nodes = V.DeviceNodes(63 * rows + 4369, device=dev)

                def plain(bt):
                    a.apply_device(*bt, out_root=root, counts=cnt8, stream=s)

                def storing(bt):
                    b.apply_nodes_device(*bt, nodes=nodes, out_root=root2, counts=cnt8b, stream=s)
                a.info()
                b.info()  # the host's bound of the count is exact again: no apply below waits
                agree, tp, te, written = True, [], [], []
                for i in range(args.calls + 2):
                    bt = make_batch()
                    torch.cuda.synchronize()
                    t1 = timed(lambda: plain(bt))
                    t2 = timed(lambda: storing(bt))
                    agree = agree and bool((root == root2).all()) and bool((cnt8 == cnt8b).all())
                    if i >= 2:
                        tp.append(t1)
                        te.append(t2)
                        written.append(int(nodes.count.item()))
                # the phase marks, each tree on batches of its own (the trees part ways here; nothing is compared after)
                pp = phase_runs(plain, make_batch)
                pe = phase_runs(storing, make_batch)
                total = int(np.median(written))
                rec = {"items_loaded": int(m), "rows": rows, "agree_with_plain_call": agree,
                       "last_counts": [int(x) for x in cnt8b.cpu().numpy()],
                       "nodes_written": {"median": total, "min": min(written), "max": max(written)},
                       "bytes_written": total * NODE_BYTES, "plain": spread(tp), "storing": spread(te)}
                if pp and pe:
                    for i, ph in ((2, "subtrees"), (3, "top")):
                        rec["plain_" + ph] = spread([p[i] for p in pp])
                        rec["storing_" + ph] = spread([p[i] for p in pe])
                rec["copy"] = copy_floor(total)
                rec["storing_minus_plain_ms"] = round(rec["storing"]["median_ms"] - rec["plain"]["median_ms"], 4)
                return rec
            out["inputs"][name] = step(name, legs)
        finally:
            a.close()
            b.close()

    measure_tree("tree_2^20/4096", on_device(SM.case_keys("random1048576", 20)), (1 << 20) + (1 << 20), 4096)
    ok = all(r["agree_with_plain_call"] for r in out["inputs"].values())
    out["agree_with_plain_calls"] = ok
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        print("a storing call's root or counts differ from the plain call's", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
