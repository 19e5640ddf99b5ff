"""Re-record tests/golden/kernel_labels.json from this tree's label functions.

The committed file was recorded at the commit named in its "parent" field, whose labels were still put
together in Python; tests/test_kernel_labels.py holds the library's labels to it.  Run this only when a label
is MEANT to change (a kernel renamed, a template argument added):  python tests/golden/gen_kernel_labels.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import kernel_label_cases as C                                   # noqa: E402
from test_kernel_labels import label_of, label_or_none           # noqa: E402

rows = [{"family": f, "args": list(a), "label": label_or_none(f, a)} for f, a in C.explicit_cases()]
head = {"parent": subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True,
                                 check=True).stdout.strip(),
        "note": "labels of the parent commit; a refused launch has label null",
        "sweeps": {f: C.sweep_digest(f, label_of) for f in C.FAMILIES}}
with open(os.path.join(HERE, "kernel_labels.json"), "w") as out:
    out.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()) + ' "rows": [\n')
    out.write(",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")
