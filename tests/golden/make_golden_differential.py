#!/usr/bin/env python3
"""The reference's results for tests/test_reference_differential.py, recorded from the *imported reference*.

    TDSA_REFERENCE=<reference tree> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_differential.py

Runs that test module with TDSA_RECORD_REFERENCE=1: every comparison is asserted live against the reference, and
tests/golden/differential.json receives, per trial of each test, a digest of the reference's values in the order the
test compares them (plus the few plain numbers the test reads from the reference's objects).  The file is replaced
only when every test passed.  DATA only.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "differential.json")


def main():
    if not os.path.isdir(os.path.join(os.environ.get("TDSA_REFERENCE", ""), "core")):
        sys.exit("set TDSA_REFERENCE to the reference tree")
    env = dict(os.environ, TDSA_RECORD_REFERENCE="1", PYTHONDONTWRITEBYTECODE="1")
    rc = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                         os.path.join("tests", "test_reference_differential.py")], cwd=ROOT, env=env).returncode
    if rc != 0:
        if os.path.exists(OUT + ".new"):
            os.remove(OUT + ".new")
        sys.exit(f"recording failed (pytest exit {rc}); {os.path.basename(OUT)} left as it was")
    os.replace(OUT + ".new", OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
