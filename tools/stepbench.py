"""The driver of the step benches: chanbench, demodbench, detectbench, historybench, measbench,
pstatbench, pulsebench, symsyncbench, corrbench, fskbench, eyebench and modqbench.  A bench lists its steps, name -> f(args) returning dict(text=[...], **figures),
and ends in main(__file__, STEPS, header).  Every step runs in a child process of its own under a time limit; the first
step that fails, prints no result or runs out of time is the last one started, and the process exits with status 1."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np


def median_us(timer, f, warm, reps):
    """(median, min, max) in us of `reps` single calls of f after `warm` calls, each between device events on the stream
    of `timer`, a handle or an engine."""
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        timer.timer_begin()
        f()
        t.append(timer.timer_end() * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def step_copy(args):
    """The box's device-to-device copy rate, which the benches state their memory floors against."""
    import torch
    x = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    x.fill_(1.0)
    for _ in range(3):
        y.copy_(x)
    t = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y.copy_(x)
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e-3)
    moved = 2 * x.numel() * 4
    return dict(copy_bps=moved / float(np.median(t)), text=[
        f"copy: 1 GiB device to device, median of {args.reps}: {moved / np.median(t) / 1e12:.2f} TB/s read + written"])


def main(script, steps, header, limit_s=240, carry=()):
    """Runs the bench `script`.  `steps`: name -> f(args), in the report's order; header(args): the report's first line;
    `limit_s`: seconds per step, one number or {step: seconds}; `carry`: the figures besides copy_bps that a step's
    result hands to the later steps, as args.<name> (--<name> on their command lines)."""
    carry = ("copy_bps",) + tuple(carry)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--step", choices=list(steps), default=None)
    ap.add_argument("--steps", default=",".join(steps), help="the steps to run, in the order above")
    for name in carry:
        ap.add_argument("--" + name.replace("_", "-"), dest=name, type=float, default=0.0)
    args = ap.parse_args()
    args.reps = max(args.reps, 20)
    if args.step:
        print("RESULT " + json.dumps(steps[args.step](args)), flush=True)
        return
    chosen = args.steps.split(",")
    if set(chosen) - set(steps):
        ap.error(f"--steps: no step named {', '.join(sorted(set(chosen) - set(steps)))}")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(header(args))
    figures, failed = dict.fromkeys(carry, 0.0), False
    for step in [st for st in steps if st in chosen]:
        limit = limit_s[step] if isinstance(limit_s, dict) else limit_s
        cmd = [sys.executable, os.path.abspath(script), "--step", step, "--reps", str(args.reps), "--warm", str(args.warm)]
        for name in carry:
            cmd += ["--" + name.replace("_", "-"), repr(figures[name])]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            say(f"{step}: no result within {limit} s; stopping")
            failed = True
            break
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            say(f"{step}: exit status {r.returncode}; stopping\n{r.stderr[-1500:]}")
            failed = True
            break
        res = json.loads(res[-1][7:])
        figures.update((name, res[name]) for name in carry if name in res)
        for ln in res["text"]:
            say(ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if failed else 0)
