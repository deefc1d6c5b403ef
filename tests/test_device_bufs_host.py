"""tsc::DeviceBufsT (csrc/tsc_common.h), the owner of every handle's device buffers: its bookkeeping over a stub allocator, as a
stand-alone host program (tests/device_bufs_check.cpp) under AddressSanitizer (with its leak check) and UBSan.  Host code only:
nothing is loaded into Python and no device is opened, so it runs where the library is built, not where a GPU is."""
import os
import subprocess

import pytest
import torch

from deeprl_signal_control_amd.build import HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(torch.cuda.is_available(), reason='host-only sanitizer check: runs on the build machine')
def test_device_bufs_bookkeeping(tmp_path):
    exe = str(tmp_path / 'device_bufs_check')
    # host code only: the sanitizers are the host compilation's (-Xarch_host), no device code is built or instrumented
    cmd = [HIPCC, '-x', 'hip', '--offload-host-only', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-Xarch_host', '-fsanitize=address,undefined',
           '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(HERE, 'device_bufs_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and 'device_bufs_check ok' in r.stdout, r.stdout + r.stderr       # a leak or a double free exits non-zero
