"""Writes tests/golden/shamap_get.json: for a few small seeded cases of
tests/shamap_get_py.py (GOLDEN_CASES) the tree, the requests and the whole
answer -- status, first, rows and leaf key per request, depth, ID, hash and leaf
mask of every row in order, and the eight counts -- by the closed form; the
reference's walks must give the same answers, or nothing is written.

  python tests/golden/make_shamap_get.py

The file pins the model against drift; the tests read the JSON only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shamap_get_py as GM  # noqa: E402


def main():
    doc = {"source": "tests/shamap_get_py.py: answer_closed, equal to answer_by_walk", **GM.golden_document()}
    with open(os.path.join(HERE, "shamap_get.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(doc["answers"]), "answers,", sum(len(a["nodes"]) for a in doc["answers"]), "rows")


if __name__ == "__main__":
    main()
