"""The direction seed's arithmetic beyond what a case table reaches (no GPU): tests/dirseed_arith_check.cpp, a stand-alone host
program over chroma_amd/csrc/dirseed_common.h, is built with the host compiler and run -- once plainly, once under the address
and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded).  It holds the truncating division to plain int64
division over every distance for the extreme numerators and at the estimate's rounding boundaries, the int32 dot product and its
clamp to int64 at the components' extremes, and the renormalised components to 16384 at the most."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


# (float-cast-overflow is named: GCC's -fsanitize=undefined does not include it)
@pytest.mark.parametrize('flags', [['-O2'], ['-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_the_truncating_division_the_dot_product_and_the_renormalisation(tmp_path, flags):
    compiler = shutil.which('c++') or shutil.which('g++')
    command = [compiler] if compiler else ['/opt/rocm/bin/hipcc', '-x', 'c++']          # (what builds the library's host units)
    program = str(tmp_path / 'dirseed_arith_check')
    subprocess.run(command + ['-std=c++17', '-ffp-contract=off'] + flags + ['-I', os.path.join(ROOT, 'chroma_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'dirseed_arith_check.cpp'), '-o', program, '-lm'], check=True, timeout=300)
    run = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok', run.stdout + run.stderr
