"""Writes tests/golden/shamap_fetch.json: for a few small seeded pairs of
tests/shamap_fetch_py.py (GOLDEN_PAIRS), against the other tree and against
none, the two roots, the eight counts and the pack -- depth, ID, hash and leaf
mask of every node -- by the set difference; the reference's walk must give the
same nodes, or nothing is written.

  python tests/golden/make_shamap_fetch.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_fetch_py as FP  # noqa: E402


def main():
    for name in FP.GOLDEN_PAIRS:
        want, have = FP.pair(name)
        for hv in (have, None):
            assert FP.pack_by_walk(want, hv)[0] == FP.pack_by_difference(want, hv), name
    doc = {"source": "tests/shamap_fetch_py.py: pack_by_difference, equal to pack_by_walk", **FP.golden_document()}
    with open(os.path.join(HERE, "shamap_fetch.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(doc["packs"]), "packs,", sum(len(p["pack"]) for p in doc["packs"]), "nodes")


if __name__ == "__main__":
    main()
