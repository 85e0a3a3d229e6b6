#!/usr/bin/env python3
"""What the decoded-key cache (STL_TUNE_KEY_CACHE) costs and saves by hit rate:
one device-resident verify of 1,048,576 GPU-signed signatures, every key
distinct (1 % with a flipped message byte), timed with HIP events on the launch
stream at

    off    the cache off (knob 0)
    h0     every key missing: the cache cleared before the call
    h50    half the keys cached: cleared, then the first half of the rows verified
    h100   every key cached by the calls before

R rounds, the four interleaved in rotating order; median ms per call, the hits
and misses stl_get_stats counted for one call of each, and each relative to
`off`.  Every bitmap must equal the expected one.

    python tools/keycache_probe.py [R]        (STL_STREAMS=1 for the serial launch)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stellard_amd import verify as V  # noqa: E402


def main():
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(os.environ.get("N", 1 << 20))
    torch.cuda.set_device(0)
    V.init(device_count=1)
    rng = np.random.default_rng(11)
    seeds = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    msgs = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    pk, sig = V.sign_batch_device(seeds, msgs)
    bad = rng.choice(n, n // 100, replace=False)
    msgs[torch.from_numpy(bad).cuda(), 0] ^= 1
    exp = np.ones(n, bool)
    exp[bad] = False
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    k_on = V.debug_tuning(V.TUNE_KEY_CACHE, -1)
    half = (n // 2) // 64 * 64

    def call(rows=n):
        V.verify_batch_device(sig[:rows], msgs[:rows], pk[:rows], out_words=words, stream=s)

    def prepare(mode):
        V.debug_tuning(V.TUNE_KEY_CACHE, 0 if mode == "off" else k_on)
        if mode in ("h0", "h50"):
            V.key_cache_clear()
        if mode == "h50":
            call(half)
        if mode == "h100":
            call()
            call()  # keys that lost their slot to a concurrent insert get one now
        torch.cuda.synchronize()

    def timed(mode):
        prepare(mode)
        before = V.get_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        call()
        b.record(s)
        torch.cuda.synchronize()
        after = V.get_stats()
        assert np.array_equal(V.words_to_bool(words, n), exp), f"{mode}: bitmap differs"
        return a.elapsed_time(b), {k: after[k] - before[k] for k in ("key_cache_hits", "key_cache_misses")}

    modes = ["off", "h0", "h50", "h100"]
    for m in modes:  # warm-up
        timed(m)
    ms = {m: [] for m in modes}
    rows = {}
    for r in range(R):
        order = modes[r % 4:] + modes[:r % 4]
        for m in (order[::-1] if r % 2 else order):
            t, rows[m] = timed(m)
            ms[m].append(t)
    V.debug_tuning(V.TUNE_KEY_CACHE, k_on)
    off = float(np.median(ms["off"]))
    out = {"n": n, "rounds": R, "settings": V.execution_settings()}
    for m in modes:
        med = float(np.median(ms[m]))
        out[m] = {"ms": round(med, 4), "vs_off": round(med / off, 4), "min": round(min(ms[m]), 4),
                  "max": round(max(ms[m]), 4), **rows[m]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
