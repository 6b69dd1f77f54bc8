#!/usr/bin/env python3
"""Generates tests/golden/reference_lines.json: the line count of every `.jl`, `.md`, `.c` and `.f` file of the reference,
numericalEFT/MCIntegration.jl v0.4.2 (paths and counts only, no content).  tests/test_docs.py checks the repository's
`file:line` citations of the reference against it.

Run:  python tests/golden/make_reference_lines.py <checkout of MCIntegration.jl v0.4.2>
"""
import json
import os
import sys

EXTENSIONS = (".jl", ".md", ".c", ".f")


def main(ref):
    lines = {}
    for root, dirs, names in os.walk(ref):
        dirs[:] = sorted(d for d in dirs if d != ".git")
        for n in sorted(names):
            if n.endswith(EXTENSIONS):
                path = os.path.join(root, n)
                with open(path, errors="replace") as fh:
                    lines[os.path.relpath(path, ref)] = sum(1 for _ in fh)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_lines.json")
    with open(out, "w") as fh:
        json.dump({"reference": "numericalEFT/MCIntegration.jl v0.4.2", "extensions": list(EXTENSIONS), "lines": lines}, fh,
                  indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
