#!/usr/bin/env python3
"""Record tests/golden/scene_records.json: rt_scene_fingerprint of every scene of tests/scene_record_common.py.

  RT_LIB_PATH=<librt_amd.so of a build of COMMIT> python tools/record_scene_records.py COMMIT

The library must be a build of COMMIT, the commit whose records the tests pin (never the tree under test: the file
would then say nothing).  The error exits are checked against the texts the tests expect while recording."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scene_record_common as src  # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40 and os.environ.get("RT_LIB_PATH"), __doc__
    fps = {}
    for name, make in src.CASES.items():
        rc, fp, err = src.fingerprint(make())
        assert rc == 0, (name, err)
        fps[name] = f"{fp:016x}"
    for name, (make, code, text) in src.ERROR_CASES.items():
        rc, _, err = src.fingerprint(make())
        assert (rc, err) == (code, text), (name, rc, err)
    out = {"commit": commit, "what": "rt_scene_fingerprint (FNV-1a 64 of the flattened scene record) per scene of "
                                     "tests/scene_record_common.py, from a build of `commit`",
           "fingerprints": fps}
    with open(os.path.join(ROOT, "tests", "golden", src.GOLDEN), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"recorded {len(fps)} fingerprints")


if __name__ == "__main__":
    main()
