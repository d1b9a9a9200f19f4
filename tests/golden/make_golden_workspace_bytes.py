"""writes tests/golden/workspace_bytes.json: what the scda_*_workspace_bytes entries of the evaluators and mask kernels answer for every
case of tests/test_workspace_bytes.py (host arithmetic, no GPU).  The file was recorded from the build before the layouts moved onto
csrc/eval_prims.h (SCDA_OPS_LIB pointing at that library).  Regenerate only when a layout is meant to move, and say which and why."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_workspace_bytes as t

got = t.answers()
with open(t.GOLDEN, "w") as f:
    f.write("{\n" + ",\n".join(' %s: %d' % (json.dumps(k), v) for k, v in got.items()) + "\n}\n")
print("%d sizes -> %s" % (len(got), t.GOLDEN))
