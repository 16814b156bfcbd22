"""The rank cell's count, one text for host and device (acf_amd/csrc/host_plan.h: rankCount), as a stand-alone program under the
address and undefined-behaviour sanitizers: tests/rank_count_main.cpp + acf_amd/csrc/host_plan.cpp, built with g++ and run as a
program of its own (nothing is preloaded).  It compares RankTables::rankOfCell with std::upper_bound on three threshold sets
(FACE80-like random thresholds, 192 consecutive floats, zeros of both signs with duplicates): every threshold and its two float
neighbours in every channel, and all 2^32 bit patterns of one channel per set, NaNs excluded.  The sweep is 3 x 2^32 table
look-ups under the sanitizers: about a minute on eight cores, the one long CPU test here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_count_against_upper_bound(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "rank_count_main")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                           os.path.join(ROOT, "tests", "rank_count_main.cpp"), os.path.join(ROOT, "acf_amd", "csrc", "host_plan.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=1800)
    print(p.stdout)
    assert p.returncode == 0, (p.stdout, p.stderr[-4000:])
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 3 and all(l.endswith(" 0 mismatches") for l in lines), lines
    assert "hasZero 0" in lines[0] and "hasZero 0" in lines[1] and "hasZero 1" in lines[2], lines
    # records with all seven slots in use were among those counted
    assert int(lines[0].split(" full records")[0].rsplit(" ", 1)[1]) > 0 and int(lines[1].split(" full records")[0].rsplit(" ", 1)[1]) > 0, lines
