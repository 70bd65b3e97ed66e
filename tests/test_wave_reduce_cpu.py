"""CPU check of the host model of the wave folds (tools/probes/wave_reduce_model.hpp: the fold tree of the reduction kernels, in the
__shfl_down form and in the LDS-free form of ls1-mardyn_amd/csrc/common.hpp): the stand-alone program
tests/hostcpp/wave_reduce_model_check.cpp, built with AddressSanitizer + UBSan, compares both forms with the serial evaluation of
lane 0's expression tree, bit for bit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_wave_fold_model_against_serial_tree(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the stand-alone check")
    exe = str(tmp_path / "wave_reduce_model_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hostcpp", "wave_reduce_model_check.cpp"), "-o", exe])
    p = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("wave_reduce_model_check ok"), p.stdout
