"""Writes tests/golden/shamap_nodes.json: a few small sets' inner nodes (depth,
ID, hash, leaf mask, a digest of the body) and what one apply to a small tree
stores, by the model of tests/shamap_nodes_py.py (golden_document); its two
statements must agree, or nothing is written.

  python tests/golden/make_shamap_nodes.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_nodes_py as NM  # noqa: E402
from tests import shamap_py as SM  # noqa: E402


def main():
    for shape, seed in NM.GOLDEN_SETS:
        keys = SM.case_keys(shape, seed)
        items, _ = SM.the_set(keys, NM._golden_leaves(keys, seed + 500))
        assert NM.nodes_closed(items) == NM.nodes_by_insertion(items), shape
    doc = NM.golden_document()
    with open(NM.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(sum(len(s["nodes"]) for s in doc["sets"]), "nodes,", len(doc["apply"]["stored"]), "stored by the apply")


if __name__ == "__main__":
    main()
