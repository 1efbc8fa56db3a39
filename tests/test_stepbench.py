"""tools/stepbench.py, the driver of the step benches, without a GPU and without the library: a stand-in bench whose steps
only record that they ran.  One child per step in the bench's order, the figures a step hands to the later ones, the
report on stdout and in --out, and what the rules for shared GPU machines rest on: after a step that fails, prints no
result or runs out of time nothing more is started, and the process exits with status 1.  Then each of the eight
benches' --help, which needs their steps wired to the driver and nothing heavy imported at module level."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = os.path.join(ROOT, "tools")

STAND_IN = '''
import os
import sys
import time

sys.path.insert(0, %r)
from stepbench import main


def ran(name):
    with open(os.environ["STAND_IN_LOG"], "a") as f:
        f.write(name + "\\n")


def first(args):
    ran("first")
    return dict(copy_bps=2.5e12, noise_us=7.25, text=["first: ran"])


def second(args):
    ran("second")
    assert (args.copy_bps, args.noise_us) == (2.5e12, 7.25)
    return dict(text=["second: " + " ".join(sys.argv[1:]), "second: two lines"])


def boom(args):
    ran("boom")
    sys.stderr.write("boom: the reason\\n")
    sys.exit(3)


def mute(args):
    ran("mute")
    os._exit(0)


def slow(args):
    ran("slow")
    time.sleep(60)
    return dict(text=["slow: woke up"])


def last(args):
    ran("last")
    return dict(text=["last: ran"])


ALL = dict(first=first, second=second, boom=boom, mute=mute, slow=slow, last=last)
STEPS = {name: ALL[name] for name in os.environ["STAND_IN_STEPS"].split(",")}

if __name__ == "__main__":
    main(__file__, STEPS, lambda args: f"stand-in: reps {args.reps}, warm {args.warm}", dict.fromkeys(ALL, 30) | dict(slow=2),
         carry=("noise_us",))
''' % TOOLS

HEADER = "stand-in: reps 20, warm 2"
SECOND = ["second: --step second --reps 20 --warm 2 --copy-bps 2500000000000.0 --noise-us 7.25", "second: two lines"]


def _run(tmp_path, steps, *options):
    """(exit status, stdout, stderr, the steps that ran in order, the report file's text) of the stand-in bench."""
    script, log, out = tmp_path / "standinbench.py", tmp_path / "ran.log", tmp_path / "made" / "here" / "report.txt"
    script.write_text(STAND_IN)
    env = dict(os.environ, STAND_IN_LOG=str(log), STAND_IN_STEPS=steps, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, str(script), "--out", str(out), "--reps", "5", "--warm", "2", *options],
                       env=env, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr, log.read_text().split(), out.read_text()


def test_steps_run_in_order_one_child_each_and_the_report_is_the_header_and_their_lines(tmp_path):
    rc, stdout, stderr, ran, report = _run(tmp_path, "first,second,last")
    assert rc == 0, stderr
    assert ran == ["first", "second", "last"]
    # --reps 5 is raised to 20, --warm and the figures of `first` reach the later steps' command lines
    assert stdout == "\n".join([HEADER, "first: ran", *SECOND, "last: ran"]) + "\n"
    assert report == stdout


def test_steps_option_selects_and_keeps_the_bench_order(tmp_path):
    rc, stdout, stderr, ran, report = _run(tmp_path, "first,second,last", "--steps", "last,first")
    assert rc == 0, stderr
    assert ran == ["first", "last"]
    assert stdout == report == "\n".join([HEADER, "first: ran", "last: ran"]) + "\n"


@pytest.mark.parametrize("bad, stopping", [
    ("boom", "boom: exit status 3; stopping\nboom: the reason\n"),
    ("mute", "mute: exit status 0; stopping\n"),
    ("slow", "slow: no result within 2 s; stopping")])
def test_nothing_starts_after_a_failed_step_and_the_exit_status_is_1(tmp_path, bad, stopping):
    rc, stdout, _, ran, report = _run(tmp_path, f"first,{bad},last")
    assert rc == 1
    assert ran == ["first", bad]
    assert stdout.split("\n")[2] == stopping.split("\n")[0]               # the third line, after the header and `first`
    assert stdout == "\n".join([HEADER, "first: ran", stopping]) + "\n"     # for boom the child's stderr tail follows it
    assert report == stdout


BENCHES = {"chan": ["copy", "bank_8_1", "bank_8_2", "bank_64_1", "bank_64_2", "bank_256_1", "bank_256_2", "spectra", "diff"],
           "demod": ["copy", "fm", "am", "split", "numpy"],
           "detect": ["copy", "second", "worst", "scale"],
           "history": ["copy", "push", "ribbon", "lines", "surface", "host"],
           "meas": ["copy", "second", "parts", "scale"],
           "pstat": ["copy", "int8", "constant", "c64", "streams", "scale"],
           "pulse": ["copy", "int8", "c64", "dense", "streams"],
           "symsync": ["copy", "tick", "second", "numpy"]}


# runs a bench as the main program in a process where importing torch or the package is an error
NOTHING_HEAVY = '''
import os, runpy, sys
class Refuse:
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in ("torch", "topdogspectrumanalyser_amd"):
            raise ImportError(name + " is imported at module level")
sys.meta_path.insert(0, Refuse())
sys.argv = sys.argv[1:]
sys.path.insert(0, os.path.dirname(sys.argv[0]))
runpy.run_path(sys.argv[0], run_name="__main__")
'''


@pytest.mark.parametrize("bench", sorted(BENCHES))
def test_each_bench_shows_its_steps_without_the_library(bench):
    r = subprocess.run([sys.executable, "-c", NOTHING_HEAVY, os.path.join(TOOLS, bench + "bench.py"), "--help"],
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    shown = " ".join(r.stdout.split())
    assert "--step {" + ",".join(BENCHES[bench]) + "}" in shown, r.stdout
    for option in ("--out", "--reps", "--warm", "--steps", "--copy-bps"):
        assert option in shown, option
