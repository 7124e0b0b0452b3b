"""visfly_amd/csrc/vf_step_consts.hpp ON THE HOST (tests/step_consts_host.cpp, built with the system compiler; no GPU):
1. the packer of the step-constant block: every word of the block equals the configuration field it copies, bit for bit, for the seven
   configurations of tests/test_constants.py.  The expected words are restated here from the layout interval_mats() arranges
   (csrc/vf_dyn_device.hpp): column k of B, the (row 1, row 2) pairs of the columns of J and Jinv, (c_motor, tm0), (tm1, tm2).
2. hit_threshold: `y < T` equals `sqrtf(y) < r` for every fp32 y within 64 ulps either side of T (y is a sum of squares, so the
   neighbourhood stops at +0), +0, the denormal extremes, +inf and NaNs, for radii that include the default 0.1, +-0, a negative, denormals,
   +inf and a NaN; T has the edge values the design states and is the smallest float whose root reaches r."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_constants import CASES
from visfly_amd import _lib
from visfly_amd.constants import derive_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    out = str(tmp_path_factory.mktemp("step_consts") / "step_consts_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "visfly_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "step_consts_host.cpp"), "-o", out])
    return out


def _u32(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def test_every_word_of_the_block_is_the_field_it_copies(exe, tmp_path):
    cfgs = [_lib.DynCfg.from_dict(derive_constants(**kw)) for kw in CASES.values()]
    path = tmp_path / "cfgs.bin"
    path.write_bytes(b"".join(bytes(c) for c in cfgs))
    out = subprocess.run([exe, "pack", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = out.stdout.strip().splitlines()
    assert len(rows) == len(cfgs) == 7
    for name, c, row in zip(CASES, cfgs, rows):
        got = np.array([int(w, 16) for w in row.split()], np.uint32)
        B, J, Ji = (np.array(list(getattr(c, f)), np.float32) for f in ("B", "J", "Jinv"))
        want = np.concatenate([_u32(B.reshape(4, 4).T.reshape(-1)),                       # Bcol[k] = column k of the row-major B
                               _u32(J.reshape(3, 3)[1:3].T.reshape(-1)),                  # J12[k] = (J[1][k], J[2][k])
                               _u32(Ji.reshape(3, 3)[1:3].T.reshape(-1)),
                               _u32([c.c_motor, c.tm0, c.tm1, c.tm2])])
        assert want.size == 32 and ctypes.sizeof(c) > 0
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want))
        assert np.any(want != 0)


def test_hit_threshold_is_the_square_root_compare(exe):
    out = subprocess.run([exe, "hit"], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    checked, bad = (int(x) for x in out.stdout.strip().splitlines()[-1].split()[1::2])
    assert bad == 0 and checked > 14 * 8 + 8 * 65
