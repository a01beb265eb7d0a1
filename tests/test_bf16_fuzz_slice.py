"""One seeded slice of each fuzzer in bfloat16 (tools/fuzz_session.py --bf16, tools/fuzz_replay.py --bf16), run as the fp16 slices of
tests/test_fuzz_slices.py are: a child process, ~25 s of fuzzing, the verdict line checked.  In bf16 the fuzzers hold window-plan
sessions, the eager path and every replay step to the a-priori bound of the kernels' arithmetic against fp64 truth
(tools/error_bound.py); legacy sessions stay bit for bit."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(script, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", script), *map(str, args)], capture_output=True, text=True,
                       timeout=420, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.strip().splitlines()[-1]


def test_session_fuzzer_slice_bf16():
    line = _run("fuzz_session.py", 25, 31, "mix", "--bf16")
    print(line)
    assert line.startswith("session fuzz bf16 ok:"), line
    trees, steps = int(line.split()[4]), int(line.split("),")[1].split()[0])
    assert trees >= 3 and steps >= 100, line  # (a slice that fuzzed nothing proves nothing)
    assert float(line.split("err / bound")[1].split(")")[0]) <= 1.0, line


def test_replay_fuzzer_slice_bf16():
    line = _run("fuzz_replay.py", 25, 31, "--bf16")
    print(line)
    assert line.startswith("fuzz bf16 ok:"), line
    assert int(line.split()[3]) >= 3 and float(line.split("err / bound")[1].rstrip(")")) <= 1.0, line
