"""The flush's decisions (goworld_amd/csrc/gwaoi_plan.h: FlushFacts -> FlushPlan): tests/cpp/plan_test.cpp
includes the header alone (no HIP) and checks named flushes against values written out by hand, then
the implications between the decisions over every combination of the boolean facts."""
import subprocess

from goworld_amd import build


def test_flush_plan_standalone():
    exe = build.build_plan_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
