"""tools/device_code_diff.py (is the device code of two builds the same, kernel by kernel) on a two-kernel toy cross-compiled for
gfx950: no GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
TOOL = os.path.join(ROOT, "tools", "device_code_diff.py")

TOY = r'''
#include <hip/hip_runtime.h>
extern "C" __global__ void toy_scale(const float* a, float* o, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] * %s;
}
extern "C" __global__ void toy_sum(const double* a, double* o, int n)
{
    double s = 0;
    for (int j = threadIdx.x; j < n; j += 64) s += a[j];
    o[threadIdx.x] = s;
}
'''


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_same_source_is_identical_and_one_changed_literal_differs_in_its_kernel_only(tmp_path):
    libs = {}
    for name, literal in (("a", "3.0f"), ("same", "3.0f"), ("other", "5.0f")):
        src = tmp_path / (name + ".hip")
        src.write_text(TOY % literal)
        libs[name] = str(tmp_path / ("lib%s.so" % name))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-o", libs[name], str(src)], stderr=subprocess.DEVNULL)

    def run(x, y):
        r = subprocess.run([sys.executable, TOOL, libs[x], libs[y]], capture_output=True, text=True)
        rows = dict(reversed(l.split()[:2]) for l in r.stdout.split("\n") if l and not l.startswith("#"))
        return r.returncode, rows, r.stdout

    code, rows, out = run("a", "same")
    assert code == 0 and rows == {"toy_scale": "identical", "toy_sum": "identical"}, out
    assert "# 2 kernels: 2 identical, 0 allocation-only, 0 differs" in out
    code, rows, out = run("a", "other")
    assert code == 1 and rows == {"toy_scale": "differs", "toy_sum": "identical"}, out
