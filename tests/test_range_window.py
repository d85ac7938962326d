"""The cell window of a range read holds every hit (csrc/gwaoi_range.h): the stand-alone program
tests/cpp/range_test.cpp includes the header alone, draws more than 10^7 (grid, centre, radius,
candidate) cases with the adversarial ones among them and checks that a candidate for which the
hit predicate holds always lies in a cell of the window.  No GPU."""
import subprocess

from goworld_amd import build


def test_range_window_holds_every_hit_standalone():
    exe = build.build_range_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok", r.stdout
    cases, hits, margin_needed = int(words[1]), int(words[2]), int(words[4])
    assert cases >= 10_000_000 and 0 < hits < cases
    assert margin_needed > 0  # some drawn hit lies outside cell_of(c - r) .. cell_of(c + r): the margin is tested
