"""writes tests/golden/launch_plans.json and wino_plans.json: the launch decision (scda_amd/csrc/launch_plan.h, through the library's
GPU-less debug entries) of every case of tests/test_launch_plans.py.  Regenerate only when a decision is meant to move, and say which and why."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_launch_plans as t
from scda_amd import native

plans = {key: t.decide(kind, args, env) for key, kind, args, env in t.cases()}
with open(t.GOLDEN, "w") as f:
    f.write('{"fields": %s,\n "plans": {\n' % json.dumps(list(native.PLAN_FIELDS)))
    f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in plans.items()))
    f.write("\n }}\n")
print("%d plans -> %s" % (len(plans), t.GOLDEN))

plans = {key: t.decide(kind, args, env) for key, kind, args, env in t.wino_cases()}
with open(t.WINO_GOLDEN, "w") as f:
    f.write('{"fields": %s,\n "wgrad_fields": %s,\n "plans": {\n' % (json.dumps(list(native.WINO_PLAN_FIELDS)), json.dumps(list(native.WINO_WGRAD_PLAN_FIELDS))))
    f.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in plans.items()))
    f.write("\n }}\n")
print("%d Winograd plans and routes -> %s" % (len(plans), t.WINO_GOLDEN))
