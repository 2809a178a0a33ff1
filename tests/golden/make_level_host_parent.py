"""Generate tests/golden/level_host_parent.json: what the host restatements of the level
(mm_level_host, mm_album_level_host) deliver on the seeded inputs of the level's tests.

    python tests/golden/make_level_host_parent.py

The file was recorded with the library built from the commit BEFORE the two restatements came to
share one loop (its id is in the file); tests/test_level_golden.py compares today's library with
it field for field.  The cases and what is recorded of each are that module's (level_cases,
album_cases, record_all), so the generator and the test cannot drift apart.  Run it again only
to add a case, and then check that no recorded case changes.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import conftest  # noqa: E402,F401  (puts the package on the path)
import test_level_golden as tg  # noqa: E402


def main() -> None:
    commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"]).decode().strip()
    doc = {"comment": "mm_level_host and mm_album_level_host as built from `commit`, the parent of the commit that "
                      "gave them one loop: SHA-256 of every delivered track, every struct field, doubles as hex floats",
           "commit": commit, "cases": tg.record_all()}
    with open(tg.PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{tg.PATH}: {len(doc['cases'])} cases at {commit}")


if __name__ == "__main__":
    main()
