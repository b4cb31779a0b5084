"""tools/codeobj_diff.py on two builds of a two-kernel source that differ in one kernel's constant: exactly that kernel is
reported as different, the other as the same, and the exit status says so.  Cross-compiles for gfx950; needs no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

SRC = """#include <hip/hip_runtime.h>
__global__ void k_scale(float* x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] *= SCALE;
}
template <int STEP>
__global__ void k_shift(float* x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += float(STEP);
}
template __global__ void k_shift<3>(float*, int);
"""


def diff(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "codeobj_diff.py"), *args], capture_output=True, text=True)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_codeobj_diff_names_exactly_the_changed_kernel(tmp_path):
    (tmp_path / "k.hip").write_text(SRC)
    builds = []
    for side, scale in (("parent", "2.0f"), ("branch", "2.5f")):
        (tmp_path / side).mkdir()
        builds.append(subprocess.Popen([HIPCC, "-O3", "--offload-arch=gfx950", f"-DSCALE={scale}", "-c", str(tmp_path / "k.hip"),
                                        "-o", str(tmp_path / side / "k.o")]))
    assert [b.wait() for b in builds] == [0, 0]
    r = diff(str(tmp_path / "parent"), str(tmp_path / "branch"))
    lines = r.stdout.splitlines()
    assert r.returncode == 1, r.stdout + r.stderr
    scale = [l for l in lines if "k_scale(" in l]
    shift = [l for l in lines if "k_shift<3>(" in l]
    assert len(scale) == 1 and scale[0].startswith("DIFFERENT"), r.stdout
    assert len(shift) == 1 and shift[0].startswith("same"), r.stdout
    assert "vgpr" in shift[0] and "scratch 0" in shift[0] and "size" in shift[0]
    assert lines[-1] == "kernels: 1 same, 1 DIFFERENT, 0 ADDED, 0 REMOVED"
    assert any(l.strip().startswith("mnemonics parent - branch:") for l in lines)
    # a build against itself: nothing changed, exit status 0; an object on one side only: its kernels are ADDED
    same = diff(str(tmp_path / "parent"), str(tmp_path / "parent"), "--objects", "k.o")
    assert same.returncode == 0 and same.stdout.splitlines()[-1] == "kernels: 2 same, 0 DIFFERENT, 0 ADDED, 0 REMOVED"
    (tmp_path / "empty").mkdir()
    added = diff(str(tmp_path / "empty"), str(tmp_path / "branch"), "--objects", "k.o")
    assert added.returncode == 1 and added.stdout.splitlines()[-1] == "kernels: 0 same, 0 DIFFERENT, 2 ADDED, 0 REMOVED"
