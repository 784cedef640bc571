"""The chunk arithmetic of the staged host uploads (csrc/stage_chunks.h) without a device: stage_chunks_check.cpp, beside this
file, includes only that header, walks the chunks of a table of block shapes and checks that they tile the rows exactly once
and in order, that no copy reads past the host block or writes past the staging buffer, and that a chunk has at least one row."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANGXX = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')


def test_stage_chunks_tile_the_rows_within_source_and_staging_buffer(tmp_path):
    if not os.path.exists(CLANGXX):
        pytest.skip("the ROCm toolchain's host compiler is missing: %s" % CLANGXX)
    exe = str(tmp_path / 'stage_chunks_check')
    subprocess.run([CLANGXX, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', os.path.join(HERE, 'stage_chunks_check.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'stage chunks ok' in r.stdout
