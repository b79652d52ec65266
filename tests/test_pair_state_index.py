"""
The record index of the pair state table (csrc/common.h: pair_state_record) on the host: tools/pair_state_index_check.cpp
enumerates every (trajectory, e, s, sn, sm, t1, g1, q2) of small sets and checks that the index is a bijection onto the records
ensure_pairs allocates.  Built with AddressSanitizer and UBSan as a program of its own: no GPU, nothing loaded into Python.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_state_index_is_a_bijection(tmp_path):
    cxx = next((c for c in ('g++', 'clang++', 'c++') if shutil.which(c)), None)
    assert cxx is not None, 'no host C++ compiler'
    exe = str(tmp_path / 'pair_state_index_check')
    # (the sanitizer's runtime linked statically: the program then runs whatever else the environment loads in front of it)
    static = ['-static-libasan', '-static-libubsan'] if cxx == 'g++' else []
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', *static,
                    '-I', os.path.join(ROOT, 'bild_amd', 'csrc'), os.path.join(ROOT, 'tools', 'pair_state_index_check.cpp'), '-o', exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert '0 failed' in run.stdout
