"""The owning buffer types of goworld_amd/csrc/gwaoi_mem.h (device and pinned buffers, events,
streams): tests/cpp/mem_test.cpp includes the header alone and links only the HIP runtime.
Without a device every allocation fails cleanly, so it checks the failure states (non-zero
status, empty object, no-op reset, moves, all-or-nothing groups); with one it checks the same
properties on live allocations."""
import subprocess

from goworld_amd import build


def test_mem_types_standalone():
    exe = build.build_mem_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok"
