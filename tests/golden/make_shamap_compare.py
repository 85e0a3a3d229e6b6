"""Writes tests/golden/shamap_compare.json from the model of
tests/shamap_lookup_py.py: a few small pairs of maps with the rows and counts
of their compare, and per pair a handful of lookups against map a.

    python -m tests.golden.make_shamap_compare

The pairs come from shamap_lookup_py.pair (seeded); the file stores them in
full, so it pins the model and the pairs both."""
import json
import os

import numpy as np

from tests import shamap_lookup_py as LM

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shamap_compare.json")
NAMES = ["empty", "vs_empty", "one_of_each", "bucket_1_1", "bucket_1_2", "shared_3_4_63"]
MAX_ROWS = 4  # below |D| for some pairs, above for others


def main():
    doc = {"max_rows": MAX_ROWS, "pairs": []}
    for name in NAMES:
        a, b = LM.pair(name)
        rows, counts = LM.compare(a, b, 1 << 20)
        first, _ = LM.compare(a, b, MAX_ROWS)
        assert rows == LM.brute_compare(a, b) and first == rows[:MAX_ROWS]
        rng = np.random.default_rng(900 + NAMES.index(name))
        queries = sorted(a)[:3] + sorted(set(b) - set(a))[:3] + LM._rand(rng, 2)
        found, leaf, pos = LM.lookup(a, queries)
        doc["pairs"].append({
            "name": name,
            "a": [[k.hex(), v.hex()] for k, v in sorted(a.items())],
            "b": [[k.hex(), v.hex()] for k, v in sorted(b.items())],
            "rows": [[k.hex(), kind, la.hex(), lb.hex()] for k, kind, la, lb in rows],
            "counts": counts,
            "lookup": [[q.hex(), f, l.hex(), p] for q, f, l, p in zip(queries, found, leaf, pos)],
        })
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
