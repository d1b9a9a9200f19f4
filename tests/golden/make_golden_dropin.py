"""Generates tests/golden/dropin_ref_params.json: for every callable the drop-in replaces, the positional parameter names (without
self / ctx) of its definition in the REFERENCE's sources, read with `ast` from the reference checkout:

    SCDA_REFERENCE=<reference checkout> python tests/golden/make_golden_dropin.py

The callables are the keys of the signature table in tests/test_dropin_imports.py's PROBE ("<reference file>:<qualified name>")."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import test_dropin_imports as T
    r = subprocess.run([sys.executable, "-c", T.PROBE, ROOT, T.REF], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=""))
    line = [l for l in r.stdout.splitlines() if l.startswith("PROBE")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-4000:]
    keys = json.loads(line[0][5:])["sigs"]
    want = {k: T.reference_params(*k.split(":")) for k in keys}
    with open(os.path.join(HERE, "dropin_ref_params.json"), "w") as f:
        json.dump(want, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(want), "callables")


if __name__ == "__main__":
    main()
