"""Writes tests/golden/shamap_roots.json: for each (shape, seed) of
tests/shamap_py.py's GOLDEN_CASES the SHAMap root and the four counts the model
gives for case_keys(shape, seed), by both of its statements (the recursive
definition and the insertion walk must agree, or nothing is written).

  python tests/golden/make_shamap.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_py as SM  # noqa: E402


def main():
    cases = []
    for shape, seed in SM.GOLDEN_CASES:
        keys = SM.case_keys(shape, seed)
        root, counts = SM.model(keys)
        walk = SM.root_by_insertion((k.tobytes(), k.tobytes()) for k in keys)
        assert walk == (root, counts[2], counts[3], counts[1]), shape
        cases.append({"shape": shape, "seed": seed, "n": int(keys.shape[0]), "root": root.hex(), "counts": counts})
    doc = {"source": "tests/shamap_py.py: root_recursive == root_by_insertion; leaf hash = key",
           "cases": cases}
    with open(os.path.join(HERE, "shamap_roots.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
