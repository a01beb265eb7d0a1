"""One seeded slice of tools/fuzz_session.py --kv8 per element type, run as tests/test_bf16_fuzz_slice.py runs its slices: a child process,
~25 s of fuzzing, the verdict line checked.  The fuzzer decodes random trees and forests over fp8 KV pools (random per-head scales, every
unused slot a NaN code) through deft_amd.DecodeSession -- one form of a layer per run, fused or two launches -- against the eager path:
pool bytes and page tables bit for bit, legacy sessions bit for bit, window plans by the 16-bit session's rules, and both sides against
fp64 truth over the dequantised pool at every step."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_session.py"), *map(str, args)], capture_output=True, text=True,
                       timeout=420, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.strip().splitlines()[-1]


def _verdict(line, elem):
    print(line)
    assert line.startswith("session fuzz kv8 ok:"), line
    trees, steps = int(line.split()[4]), int(line.split("),")[1].split()[0])
    assert trees >= 3 and steps >= 100, line  # (a slice that fuzzed nothing proves nothing)
    assert f"elements {elem}" in line, line
    assert float(line.split("worst err / tol")[1].split(")")[0]) <= 1.0, line
    return line


def test_session_fuzzer_slice_kv8():
    _verdict(_run(25, 31, "mix", "--kv8"), "fp16")


def test_session_fuzzer_slice_kv8_bf16():
    line = _verdict(_run(25, 31, "mix", "--kv8", "--bf16"), "bf16")
    assert float(line.split("worst err / bound")[1].split(";")[0]) <= 1.0, line
