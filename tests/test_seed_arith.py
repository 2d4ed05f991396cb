"""The vertex seed's arithmetic beyond what its calls can be handed (no GPU): tests/seed_arith_check.cpp, a stand-alone host
program over chroma_amd/csrc/seed_common.h, is built with the host compiler and run -- once plainly, once under the address and
undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded).  It holds the floor square root to its
definition on (y^2 + 1)^2 - 1 for every y up to 2^53 (y = 5791 and 5792 among them: differences the coordinate ranges of
chroma_vertex_seed do not admit), the settling compares on estimates one off, and the cutting of a batch into launches of fewer
than 2^32 threads."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


# (float-cast-overflow is named: GCC's -fsanitize=undefined does not include it)
@pytest.mark.parametrize('flags', [['-O2'], ['-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_the_floor_square_root_and_the_launch_cuts(tmp_path, flags):
    compiler = shutil.which('c++') or shutil.which('g++')
    command = [compiler] if compiler else ['/opt/rocm/bin/hipcc', '-x', 'c++']          # (what builds the library's host units)
    program = str(tmp_path / 'seed_arith_check')
    subprocess.run(command + ['-std=c++17', '-ffp-contract=off'] + flags + ['-I', os.path.join(ROOT, 'chroma_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'seed_arith_check.cpp'), '-o', program, '-lm'], check=True, timeout=300)
    run = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok', run.stdout + run.stderr
