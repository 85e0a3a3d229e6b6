"""Writes tests/golden/shamap_fork.json: for each small seeded case of
tests/shamap_fork_py.py (CASES) the source tree, the batch's size, and the roots
of both trees after the fork with the eight counts, by the model (the source's
root is the one it had: a fork only reads it).  Every root is also computed by
the bucket recurrence stated on its own (root_by_buckets); the two must agree,
or nothing is written.

  python tests/golden/make_shamap_fork.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_fork_py as FM  # noqa: E402
from tests import shamap_tree_py as TM  # noqa: E402


def main():
    cases = []
    for name in FM.CASES:
        src, batch = FM.case(name)
        before = dict(src.items)
        dst, root, counts = FM.fork(src, *batch)
        assert src.items == before, name
        assert TM.root_by_buckets(dst.items) == root and TM.root_by_buckets(src.items) == src.root(), name
        cases.append({"name": name, "source_items": len(src.items), "rows": int(len(batch[0])),
                      "source_root": src.root().hex(), "fork_root": root.hex(), "counts": counts})
    doc = {"source": "tests/shamap_fork_py.py: fork = shamap_tree_py.Model copied, then applied", "cases": cases}
    with open(os.path.join(HERE, "shamap_fork.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
