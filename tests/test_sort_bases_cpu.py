"""sqz_amd/csrc/sort_bases.h on the host: index_sort_kernel counts one digit per position and derives the histograms
of its passes 1 and 2 from that of pass 0.  The kernel has 16 waves and the wave emulator runs 8 (tests/emu), so the
header -- which the kernel calls and keeps no second copy of -- is what can be held against a reference without a GPU:
tests/harness/sort_bases_check.cpp, built with the address and undefined-behaviour sanitizers, counts pass 0's histogram
directly, derives the other two through the header and compares all three with histograms counted from the keys.
Both splits; every n from 4 to 40, 4097, 4098, 4099, 50001; uniform random bytes, bytes 0x00..0x04 only, all 0xFF, and
four blocks per length that differ in their first two and last two bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "sort_bases_check.cpp")


def test_derived_histograms_equal_the_counted_ones(tmp_path):
    exe = str(tmp_path / "sort_bases_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-2000:] + p.stderr[-4000:]
