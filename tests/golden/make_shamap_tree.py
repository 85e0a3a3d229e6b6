"""Writes tests/golden/shamap_tree_roots.json: for each seeded batch sequence of
tests/shamap_tree_py.py (SEQUENCES) the root and the eight counts the model
gives after every step.  The root of every step is also computed by the bucket
recurrence stated on its own (root_by_buckets); the two must agree, or nothing
is written.

  python tests/golden/make_shamap_tree.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_tree_py as TM  # noqa: E402


def main():
    seqs = []
    for name in TM.SEQUENCES:
        m, steps = TM.Model(), []
        for b in TM.sequence(name):
            root, counts = m.apply(*b)
            assert TM.root_by_buckets(m.items) == root, name
            steps.append({"rows": int(len(b[0])), "root": root.hex(), "counts": counts})
        seqs.append({"name": name, "steps": steps})
    doc = {"source": "tests/shamap_tree_py.py: Model over shamap_py.model == root_by_buckets",
           "sequences": seqs}
    with open(os.path.join(HERE, "shamap_tree_roots.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(seqs), "sequences", sum(len(s["steps"]) for s in seqs), "steps")


if __name__ == "__main__":
    main()
