#!/usr/bin/env python3
"""profiles/path_a_products.json from the figures tests/test_gpu_path_a_products.py prints before it asserts:

    python -m pytest -q -s -m gpu tests/test_gpu_path_a_products.py | python tools/path_a_products_figures.py

Per implementation (hh_pa nearest neighbour / trilinear, the batch's sliced, general, lds, factored and banded forms): the number
of cases, the largest normalised error max |got - ref| / max(1, max |ref|) against the float64 oracle matrix over four
probes each way, and the case it belongs to."""
import json
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent.parent / "profiles" / "path_a_products.json"


def main():
    worst = {}
    for line in sys.stdin:
        at = line.find("path_a_products figure ")   # (pytest -q puts its progress dots in front of a test's first line)
        if at < 0:
            continue
        name, value, case = line[at:].split()[2:5]
        value = float(value)
        w = worst.setdefault(name, {"cases": 0, "max_normalised_error": 0.0, "at": None})
        w["cases"] += 1
        if value >= w["max_normalised_error"]:
            w["max_normalised_error"], w["at"] = value, case
    if not worst:
        sys.exit("no 'path_a_products figure' lines on stdin (run pytest with -s)")
    doc = {"what": "Path A products against the float64 oracle matrix [A_data; A_hsym], tests/test_gpu_path_a_products.py, MI355X",
           "bound": 1e-12, "implementations": dict(sorted(worst.items()))}
    OUT.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
