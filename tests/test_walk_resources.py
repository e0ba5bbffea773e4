"""The register budget of the nearest-triangle search as its own launch (query_kernels.hip: k_nearest<LATTICE, ALT, CLAMP>): the
walk hides its dependent scalar loads behind 8 waves per SIMD, so every instantiation stays at <= 64 VGPRs, without scratch and
without a spilled register, scalar ones included (gfx950: 102 allocatable SGPRs; the remark counts VCC and the reserved ones on
top, and a kernel that needs more spills, which the remark reports separately).  No GPU: hipcc's resource remarks, read by
tools/kernel_resources.py."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_k_nearest_instantiation_keeps_eight_waves():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {k: v for k, v in mod.remarks("query_kernels.hip").items() if k.startswith("_ZN4icon9k_nearestILb")}
    # the 257^3 launch (clamped, on boxes known to be there), the lattice launch that asks the mesh (plain / the alternative tie rule),
    # Morton point packets (plain / the alternative tie rule)
    assert sorted(k[len("_ZN4icon9k_nearestI"):].split("EEEv")[0] for k in res) == sorted(
        ["Lb1ELb0ELb1", "Lb1ELb0ELb0", "Lb1ELb1ELb0", "Lb0ELb0ELb0", "Lb0ELb1ELb0"]), sorted(res)
    for k, v in res.items():
        print(k[:60], v)
        assert v["VGPRs"] <= 64 and v["Occupancy"] == 8, (k, v)
        assert v["ScratchSize"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["TotalSGPRs"] <= 102 + 6, (k, v)
