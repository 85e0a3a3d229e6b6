"""Registered signer sets against the per-batch key dedup, device-resident,
in one process: S signers sign `rows` messages (seeded, made on the device
with sign_batch_device; one row in 16 is broken so the bits are not all ones),
and three legs verify them, alternating A A' B B A' A:

    A   verify_batch_device(..., DEDUP_KEYS)      the key domain built per call
    A'  verify_batch_device(...)                  the automatic choice
    B   Keyset.verify_batch_device                tables built once, at registration

The bits of the three legs are compared first; any difference fails the run.
Then: warm-up, and R rounds of that order (2 R timed calls per leg, R >= 10),
each call between two device events.  Also: leg B for 16, 1,000 and 4,096
registered signers (tables of 8.5 MiB to 2 GiB), a 1,000-row call's latency
(host clock around call + synchronize) for A and B, and stl_keyset_create's
time for 1,000 keys.  Every step runs under its own time limit (--step-timeout
seconds): a step that overruns ends the process with status 124 before
anything else is started.  Prints one JSON line (kept as
profiles/keyset/bench.json).

    python3 tools/keyset_bench.py [--rows N] [--rounds R] [--step-timeout S] [--out FILE]

With --by-key the tool measures the calls that take public keys instead (see
by_key below; kept as profiles/keyset/by_key.json).
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


def spread(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
            "max_ms": round(float(a.max()), 4), "calls": int(a.size)}


def by_key(args, out, step, timed, V, torch, keys_all, who, pk, sig, msg, s):
    """--by-key: the same S signers x rows, five legs alternating a b c d e e d c b a:

        a  Keyset.verify_batch_device            indices given
        b  Keyset.verify_by_key_device           every signer registered (0 misses)
        c  Keyset.verify_by_key_device           one signer in 16 left out of the set
        d  Keyset.verify_by_key_device           none of the signers registered
        e  verify_batch_device                   the per-signature call, automatic choice

    All legs verify the same rows, so their bits are compared directly before
    timing.  Also timed, outside the alternation: the lookup kernel alone
    (lookup_device), which with the call's one wait is what b adds to a."""
    n, S = sig.shape[0], args.signers
    dev = sig.device
    out["tool"] = "keyset_bench --by-key"
    keys = keys_all[:S].cpu().numpy()
    keep = np.arange(S) % 16 != 0
    others = keys_all[S:2 * S].cpu().numpy() if keys_all.shape[0] >= 2 * S else keys_all[S:].cpu().numpy()
    sets = step("create", lambda: {"all": V.Keyset(keys), "most": V.Keyset(keys[keep]), "none": V.Keyset(others)})
    words = {k: torch.empty((n + 63) // 64, dtype=torch.int64, device=dev) for k in "abcde"}
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    misses = {}

    def by(name, leg):
        def fn():
            misses[leg] = sets[name].verify_by_key_device(pk, sig, msg, out_words=words[leg], stream=s)[1]
        return fn
    legs = {
        "a_indexed": lambda: sets["all"].verify_batch_device(who, sig, msg, out_words=words["a"], stream=s),
        "b_by_key_0_misses": by("all", "b"),
        "c_by_key_1_in_16": by("most", "c"),
        "d_by_key_all_misses": by("none", "d"),
        "e_per_signature": lambda: V.verify_batch_device(sig, msg, pk, out_words=words["e"], stream=s),
    }

    def bits_equal():
        for fn in legs.values():
            fn()
            fn()  # the automatic choice follows the previous call's sample
        torch.cuda.synchronize()
        exp = np.ones(n, dtype=bool)
        exp[::16] = False
        got = [V.words_to_bool(words[k], n) for k in "abcde"]
        return bool(all(np.array_equal(g, exp) for g in got)), int(got[0].sum())
    same, accepted = step("bits", bits_equal)
    out["bits_equal"], out["accepted"] = same, accepted
    out["misses"] = {"b": misses["b"], "c": misses["c"], "d": misses["d"]}
    if not same or misses["b"] != 0 or misses["d"] != n or not 0 < misses["c"] < n // 8:
        print(json.dumps(out))
        print("the legs' bits or miss counts are wrong", file=sys.stderr)
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
    out["b_minus_a_ms"] = round(med["b_by_key_0_misses"] - med["a_indexed"], 4)
    out["b_over_a"] = round(med["b_by_key_0_misses"] / med["a_indexed"], 4)
    out["c_over_e"] = round(med["c_by_key_1_in_16"] / med["e_per_signature"], 4)
    out["d_over_e"] = round(med["d_by_key_all_misses"] / med["e_per_signature"], 4)

    def lookup_only():
        fn = lambda: sets["all"].lookup_device(pk, out_index=idx, stream=s)  # noqa: E731
        fn()
        fn()
        torch.cuda.synchronize()
        return [timed(fn) for _ in range(2 * args.rounds)]
    out["lookup_kernel"] = spread(step("lookup", lookup_only))
    for ks in sets.values():
        ks.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default="")
    ap.add_argument("--by-key", action="store_true", help="the by-key legs (kept as profiles/keyset/by_key.json)")
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("--rounds >= 10 (20 timed calls per leg)")
    import torch
    from stellard_amd import build, verify as V
    signal.signal(signal.SIGALRM, _alarm)
    n = args.rows
    dev = torch.device("cuda", 0)
    out = {"tool": "keyset_bench", "rows": n, "signers": args.signers, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest()[:16]}

    def step(name, fn):
        signal.alarm(args.step_timeout)
        try:
            r = fn()
            torch.cuda.synchronize()
            return r
        except StepTimeout:
            print(f"step {name!r} overran {args.step_timeout} s", file=sys.stderr, flush=True)
            os._exit(124)
        finally:
            signal.alarm(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step("init", V.init)
    s = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0A11)
    max_keys = 4096
    base = torch.randint(0, 256, (max_keys, 32), dtype=torch.uint8, device=dev, generator=g)
    msg = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
    who_any = torch.randint(0, 1 << 30, (n,), dtype=torch.int64, device=dev, generator=g)
    keys_all = step("keys", lambda: V.sign_batch_device(base, torch.zeros_like(base))[0])
    words = [torch.empty((n + 63) // 64, dtype=torch.int64, device=dev) for _ in range(3)]

    def rows_for(nkeys):
        who = (who_any % nkeys).to(torch.int32)
        pk, sig = V.sign_batch_device(base[who.long()].contiguous(), msg)
        sig[::16, 1] ^= 1
        return who.contiguous(), pk, sig

    def make_keyset(nkeys):
        keys = keys_all[:nkeys].cpu().numpy()
        t0 = time.perf_counter()
        ks = V.Keyset(keys)
        return ks, (time.perf_counter() - t0) * 1e3

    # ---- the signer shape of configs[0] / configs[4]: S signers x rows ----
    S = args.signers
    who, pk, sig = step("rows", lambda: rows_for(S))
    if args.by_key:
        by_key(args, out, step, timed, V, torch, keys_all, who, pk, sig, msg, s)
        return
    creates = []
    for _ in range(3):
        ks, ms = step("create", lambda: make_keyset(S))
        creates.append(ms)
        ks.close()
    ks, ms = step("create", lambda: make_keyset(S))
    creates.append(ms)
    out["create_ms"] = {"keys": S, **spread(creates)}
    out["table_bytes"] = ks.info()["table_bytes"]
    legs = {
        "A_dedup": lambda w=words[0]: V.verify_batch_device(sig, msg, pk, out_words=w, policy=V.DEDUP_KEYS, stream=s),
        "A_auto": lambda w=words[1]: V.verify_batch_device(sig, msg, pk, out_words=w, stream=s),
        "B_keyset": lambda w=words[2]: ks.verify_batch_device(who, sig, msg, out_words=w, stream=s),
    }

    def bits_equal():
        for fn in legs.values():
            fn()
            fn()  # the automatic choice follows the previous call's sample
        torch.cuda.synchronize()
        exp = torch.ones(n, dtype=torch.bool)
        exp[::16] = False
        got = [V.words_to_bool(w, n) for w in words]
        return bool(np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]) and
                    np.array_equal(got[0], exp.numpy())), int(got[2].sum())
    same, accepted = step("bits", bits_equal)
    out["bits_equal"] = same
    out["accepted"] = accepted
    if not same:
        print(json.dumps(out))
        print("the legs' bits differ", file=sys.stderr)
        sys.exit(1)

    def ab():
        ts = {k: [] for k in legs}
        for k in legs:  # warm-up
            legs[k]()
            legs[k]()
        torch.cuda.synchronize()
        order = ["A_dedup", "A_auto", "B_keyset", "B_keyset", "A_auto", "A_dedup"]
        for _ in range(args.rounds):
            for k in order:
                ts[k].append(timed(legs[k]))
        return ts
    ts = step("ab", ab)
    out["legs"] = {k: spread(v) for k, v in ts.items()}
    a, b = out["legs"]["A_dedup"]["median_ms"], out["legs"]["B_keyset"]["median_ms"]
    out["B_over_A_dedup"] = round(b / a, 4)
    out["B_over_A_auto"] = round(b / out["legs"]["A_auto"]["median_ms"], 4)
    out["B_sigs_per_s"] = round(n / (b * 1e-3))

    # ---- a 1,000-row call's latency ----
    def latency():
        m = 1000
        w = [torch.empty((m + 63) // 64, dtype=torch.int64, device=dev) for _ in range(2)]
        who1, sig1, msg1, pk1 = who[:m].contiguous(), sig[:m].contiguous(), msg[:m].contiguous(), pk[:m].contiguous()
        small = {"A_dedup": lambda: V.verify_batch_device(sig1, msg1, pk1, out_words=w[0], policy=V.DEDUP_KEYS, stream=s),
                 "A_auto": lambda: V.verify_batch_device(sig1, msg1, pk1, out_words=w[0], stream=s),
                 "B_keyset": lambda: ks.verify_batch_device(who1, sig1, msg1, out_words=w[1], stream=s)}
        res = {k: [] for k in small}
        for k in small:
            small[k]()
            small[k]()
        torch.cuda.synchronize()
        for _ in range(2 * args.rounds):
            for k in small:
                t0 = time.perf_counter()
                small[k]()
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3)
        return {k: spread(v) for k, v in res.items()}
    out["latency_1000_rows"] = step("latency", latency)
    ks.close()

    # ---- table size: 16 / 1,000 / 4,096 registered signers ----
    out["by_nkeys"] = {}
    for nkeys in (16, 1000, 4096):
        whoK, _, sigK = step("rows", lambda: rows_for(nkeys))
        ksK, ms = step("create", lambda: make_keyset(nkeys))
        fn = lambda: ksK.verify_batch_device(whoK, sigK, msg, out_words=words[2], stream=s)  # noqa: E731

        def leg():
            fn()
            fn()
            torch.cuda.synchronize()
            return [timed(fn) for _ in range(2 * args.rounds)]
        r = spread(step("nkeys", leg))
        r["table_bytes"] = ksK.info()["table_bytes"]
        r["create_ms"] = round(ms, 3)
        r["accepted"] = int(V.words_to_bool(words[2], n).sum())
        out["by_nkeys"][str(nkeys)] = r
        ksK.close()
        del whoK, sigK
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
