"""The one runner of the suite's child processes.  A GPU scenario runs in a fresh process (tests/*_child.py) under a time limit, one at a
time.  On a shared GPU machine the rule is: after a fault, start nothing more.  So the first child that dies -- by a signal, an abort,
its time limit, or with a GPU fault in its output -- goes on CRASHED, and every later run_child of the session, from whichever test
module, fails at once without starting a process.  pytest imports this module once per session: one list.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CRASHED = []               # the first child that died: nothing more is started after it
DEATHS = (124, 134, 137, 139)          # time limit (timeout), abort, kill, segmentation fault, as a shell reports them
GPU_FAULTS = ("an illegal memory access was encountered", "Memory access fault by GPU", "HSA_STATUS_ERROR")


def run_child(child, scenario, *args, timeout, crashed=CRASHED, **opt):
    """`python <child> <scenario> <args...> [json of opt]` in a fresh process; returns its output (stdout + stderr, ftgp_create's
    FTGP_VERBOSE lines among it).  A scenario without positional arguments always gets its options object, an empty one too."""
    assert not crashed, f"not started: an earlier GPU scenario died ({crashed[0]}); find its cause first"
    argv = [scenario, *args] + ([json.dumps(opt)] if opt or not args else [])
    what = f"{os.path.basename(child)} {' '.join(argv)}"
    try:
        r = subprocess.run([sys.executable, child] + argv, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as x:
        crashed.append(f"{what}: no end after {timeout} s")
        out = "".join(s.decode(errors="replace") if isinstance(s, bytes) else (s or "") for s in (x.stdout, x.stderr))
        raise AssertionError(f"{crashed[0]}\n{out[-4000:]}") from None
    out = r.stdout + r.stderr
    fault = next((f for f in GPU_FAULTS if f in out), None)
    if r.returncode < 0 or r.returncode in DEATHS:
        crashed.append(f"{what}: exit status {r.returncode}")
    elif fault:
        crashed.append(f"{what}: exit status {r.returncode} with '{fault}' in its output")
    assert r.returncode == 0 and not fault, f"{crashed[0] if crashed else f'{what}: exit status {r.returncode}'}\n{out[-6000:]}"
    print(out[-3000:])
    return out
