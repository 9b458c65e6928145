"""sqz_amd/csrc/sort_rank.h on the host: index_sort_kernel ranks a row of 64 elements by one peer mask per lane -- the
lanes that hold an element with the same digit -- built from one ballot per key bit.  The kernel has 16 waves and the
wave emulator runs 8 (tests/emu), so the header -- which the kernel calls and keeps no second copy of -- is what can be
held against a reference without a GPU: tests/harness/sort_rank_check.cpp, built with the address and
undefined-behaviour sanitizers, gives it a ballot computed from all 64 lanes' digits and compares every lane's mask,
rank and count with a lane-by-lane count of equal digits.  The eight input combinations of the bit step; digits of 7,
8 and 10 bits; one digit everywhere, all different, random; all lanes valid, ragged ends, random valid masks, none."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "sort_rank_check.cpp")


def test_peer_masks_equal_the_counted_ones(tmp_path):
    exe = str(tmp_path / "sort_rank_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-2000:] + p.stderr[-4000:]
