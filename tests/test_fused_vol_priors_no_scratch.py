"""tests/test_host.py::test_hot_kernels_do_not_spill guards the six icon instantiations of k_fused_f16x3.  The body they share
with the pamir and pifu instantiations keeps its zero scratch only because four values are pinned to where they are computed
(empty `asm volatile`s in mlp_f16x3_device.h / fused_f16x3.hip / mlp_f16x3.hip: the layer-3 share of the raw inputs, the mask
flag, the lane group of layer 3, the output index) - a scheduler that moves one of them keeps up to sixteen inputs alive across
the MFMA chain.  This test holds the volume-prior instantiations to the same 0 bytes (no GPU: hipcc's resource remarks)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_fused_instantiation_is_free_of_scratch():
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as d:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "icon_amd", "csrc", "fused_f16x3.hip"), "-o", os.path.join(d, "x.o")]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:]
    scratch, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    fused = {k: v for k, v in scratch.items() if "k_fused_f16x3" in k}
    # PRIOR 0 / 1 / 2 = icon / pamir / pifu; icon: lattice, points, batch x (large, small); the volume priors: lattice, points, batch
    assert sorted(sum(f"k_fused_f16x3ILi{p}E" in k for k in fused) for p in (0, 1, 2)) == [3, 3, 6], sorted(fused)
    assert all(v == 0 for v in fused.values()), fused
