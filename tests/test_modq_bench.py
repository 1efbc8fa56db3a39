"""tools/modqbench.py is a step bench like the others: it lists its steps without importing torch or the library, and
every device step of it runs through stepbench's child processes."""
import os
import re
import subprocess
import sys

from test_stepbench import NOTHING_HEAVY, TOOLS

STEPS = ["copy", "tick", "second", "numpy"]


def test_the_bench_shows_its_steps_without_the_library():
    r = subprocess.run([sys.executable, "-c", NOTHING_HEAVY, os.path.join(TOOLS, "modqbench.py"), "--help"],
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    shown = " ".join(r.stdout.split())
    assert "--step {" + ",".join(STEPS) + "}" in shown, r.stdout
    for option in ("--out", "--reps", "--warm", "--steps", "--copy-bps"):
        assert option in shown, option


def test_the_bench_ends_in_stepbench_main_and_launches_nothing_itself():
    src = open(os.path.join(TOOLS, "modqbench.py")).read()
    assert re.search(r"^    main\(__file__, STEPS, header\)$", src, re.M)
    assert "from stepbench import main, median_us, step_copy" in src
    top = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert not [ln for ln in top if "torch" in ln or "topdogspectrumanalyser_amd" in ln], top
    assert "subprocess" not in src and "Popen" not in src


def test_the_bench_is_listed_with_the_others():
    root = os.path.dirname(TOOLS)
    assert "modqbench" in open(os.path.join(TOOLS, "stepbench.py")).read().split('"""')[1]
    assert "modqbench.py" in open(os.path.join(root, "README.md")).read()
    assert "modqbench.py" in open(os.path.join(root, "DESIGN.md")).read()
