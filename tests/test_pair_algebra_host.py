"""The register-pair algebra of the sub-step loop (visfly_amd/csrc/vf_pair_algebra.hpp) against its scalar form ON THE HOST: the plain C++
bodies of qmul_p (plain, conj(a), conj(b)), mat3_p, mat4_p and rotors_p are built with the system compiler together with the scalar qmul /
mat3 / mat4 / rotor recurrence and compared bit for bit (a NaN need only be a NaN) on 2^20 random bit patterns per operation and on every combination of
+-0, +-denormal, +-1, +-large and +-inf (tests/pair_algebra_host.cpp).  No GPU: what the device's asm bodies compute is pinned by the
oracle comparisons of tests/test_pair_algebra_gpu.py and of every fixture."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_forms_equal_scalar_forms_bit_for_bit(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    exe = str(tmp_path / "pair_algebra_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "visfly_amd", "csrc"), os.path.join(ROOT, "tests", "pair_algebra_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    checked, bad = (int(x) for x in r.stdout.strip().splitlines()[-1].split()[1::2])
    assert bad == 0 and checked == 6 * (1 << 20) + 4 * 10 ** 8 + 2 * 10 ** 6, (checked, bad)
