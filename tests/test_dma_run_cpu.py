"""CPU check of the run split of the list force pass's LDS-DMA staging (ls1-mardyn_amd/csrc/dma_run.hpp): the stand-alone program
tests/hostcpp/dma_run_check.cpp, built with AddressSanitizer + UBSan, replays the copy lane by lane over random regions."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_dma_run_split_over_random_regions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the stand-alone check")
    exe = str(tmp_path / "dma_run_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostcpp", "dma_run_check.cpp"), "-o", exe])
    p = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith("dma_run_check ok"), p.stdout
